"""TEST INFRASTRUCTURE shared by tests/test_oracle_combin_cpu.py and tests/test_gpu_combin_lattice.py: the (Fin, Fout) lattice of
combining layers (combin=True: output feature fo = sum over the Fin neurons nu = fo * Fin + fin), one case per shape-dependent
route of csrc/conv.hip, and the inputs both files run them on. Also the pooling geometry and the off() helper of
tests/test_gpu_conv_alignment.py, which moved here so that both GPU files build the same thing.

The constants the routes hang on (csrc/conv.hip, csrc/conv_mfma.h), nb = ceil(Fin * Fout / 8) blocks of 8 neurons:
  MCCNN_DF_PLANES = 4    conv_bwd_mfma<true, 3, false> (Fin = 2..4): nb <= 4 => one plane of per-edge feature-gradient sums per
                         block (df_planes), nb > 4 => ONE plane, read-modify-written (`old = (q == 0) ? 0 : *d`)
  MCCNN_LDS_MAX_NB = 64  forward: use_mfma / f1_shape take nb <= 64; beyond it the VALU kernels, and no state records
  MCCNN_WQ_BWD = 312     backward: the MFMA sweep needs (nb * 312 + 768) * 4 <= 65 536 bytes of LDS <=> nb <= 50 for a combining
                         layer (one launch, no column tiles); nb = 51..64 => conv_bwd_valu behind an MFMA forward

THE SHAPE RULE. The library keeps the reference's rule (spatial_conv.cc:290; conv.hip fill_args, MCConvModule._conv_checks,
MCConvBuilder.__native_convolution__; tests/test_gpu_native.py::test_native_path_keeps_the_ops_shape_rules): the PADDED neuron
count 8 * nb of a combining layer must be a multiple of Fin, or the call is refused (MCCNN_E_SHAPE / InvalidArgumentError) before
anything is launched. So the padding is always a whole number of output features' worth of neurons (a multiple of Fin below 8),
and some (route, shape) pairs one can write down cannot be reached by any caller:
  * Fin = 3 needs nb % 3 == 0: the last block always starts at fin 1 (r0 = 1) -- a padded last block with r0 = 0 or 2 never
    runs, nb = 4 and nb = 5 (the two sides of MCCNN_DF_PLANES) do not exist at Fin = 3; 3 -> 7 / 3 -> 6 (planes) and 3 -> 15
    (read-modify-write) are the padded shapes there are;
  * Fin > 7 is never padded (9 -> 1, 20 -> 1 are refused); Fin = 5, 6, 7 are padded by exactly Fin neurons (5 -> 7, 6 -> 3, 7 -> 7).
The nine shapes of the lattice the rule refuses (`accepted(case)` is False) stay in the table: the GPU tests assert that the op
refuses them, tests/test_oracle_combin_cpu.py that the C ABI does, and the oracle (which has no such rule) is still pinned
against float64 on them. Next to each stands the nearest accepted shape that reaches the same kernel lines.
"""
import numpy as np

from tests.helpers import make_cloud

DF_PLANES, LDS_MAX_NB, WQ_BWD = 4, 64, 312
BWD_MFMA_MAX_NB = (64 * 1024 // 4 - 4 * 192) // WQ_BWD     # 50


def block_facts(fin, fout):
    """-> (nb, neurons of the last block, r0 = fin of the last block's first neuron)"""
    neurons = fin * fout
    nb = (neurons + 7) // 8
    return nb, neurons - 8 * (nb - 1), (8 * (nb - 1)) % fin


# (Fin, Fout, nb, neurons of the last block, r0 of the last block, the route the case exists for)
# Every route the suite did not reach is named once, with "<-" in front of the kernel line it runs.
# The feature-gradient reductions hang on the same shapes (tests/test_gpu_combin_lattice.py runs both forms explicitly):
#   gather_edge_featgrad<2|3|4> / scatter_edge_featgrad with planes = 4: 2 -> 16, 4 -> 8; planes = 3: 3 -> 6, 3 -> 7, 4 -> 5;
#   planes = 1 (read-modify-write) at Fin = 2 and 4, not only 3: 2 -> 17, 2 -> 21, 4 -> 11, 4 -> 12;
#   feat_grad cleared by the ClearSpan of reduce_partials (n * Fin * 4 % 16 == 0) or by launch_zero_words, and points that are
#   nobody's neighbour at Fin > 3: 2 -> 17, 3 -> 7, 4 -> 12, 7 -> 7, 9 -> 8, 16 -> 3 on the pooling geometry (n = 909).
STATIC = [   # Fin = 2..4: conv_stream<true, 3, false> / conv_bwd_mfma<true, 3, false>, static (fin, fo) patterns
    (2, 16, 4, 8, 0, "nb == MCCNN_DF_PLANES: the widest plane form at Fin = 2 (gather / scatter with planes = 4)"),
    (2, 17, 5, 2, 0, "<- nb == 5: first read-modify-write at Fin = 2 (`old = (q == 0) ? 0 : *d`), last block 2 neurons"),
    (2, 21, 6, 2, 0, "read-modify-write, last block 2 neurons, six blocks"),
    (3, 6, 3, 2, 1, "<- planes, last block r0 = 1 with 2 neurons: NG = 3 columns from fo0 = 5 of 6, TWO of them clamped: grow[min(fo0 + k, outF - 1)]"),
    (3, 5, 2, 7, 2, "REFUSED (16 % 3). padded last block that starts at fin 2 (r0 = 2): `if (n >= numOuts) g[n] = ff[n] = 0` after combin_pick<3, 2>"),
    (3, 7, 3, 5, 1, "<- r0 = 1, 5 neurons: NG = 3 columns from fo0 = 5 of 7, the third one clamped: grow[min(fo0 + k, outF - 1)]"),
    (3, 10, 4, 6, 0, "REFUSED (32 % 3). nb == 4 at Fin = 3: planes, padded last block with r0 = 0"),
    (3, 11, 5, 1, 2, "REFUSED (40 % 3). nb == 5 at Fin = 3: read-modify-write, last block r0 = 2 with ONE neuron (fins 0, 1 untouched by it)"),
    (3, 15, 6, 5, 1, "<- Fin = 3 read-modify-write with a padded last block (the suite had 3 -> 16 alone): read-modify-write, last block r0 = 1, 5 neurons (clamp again, behind an RMW)"),
    (4, 5, 3, 4, 0, "<- Fin = 4 with a padded last block (4 of 8 neurons), planes = 3"),
    (4, 8, 4, 8, 0, "<- nb == 4 at Fin = 4: planes, full"),
    (4, 11, 6, 4, 0, "<- Fin = 4 read-modify-write (nb = 6) with a padded last block"),
    (4, 12, 6, 8, 0, "<- Fin = 4 read-modify-write, full"),
]
GENERIC = [  # Fin > 4: conv_stream<true, 0, false> / conv_bwd_mfma<true, 0, false>
    (5, 1, 1, 5, 0, "REFUSED (8 % 5). one padded block, one output feature: acc closes inside block 0"),
    (8, 1, 1, 8, 0, "one full block"),
    (5, 3, 2, 7, 3, "REFUSED (16 % 5): 5 -> 7 below runs these lines. output features straddle blocks (acc carried, closed by `++finQ == a.Fin`); fins 0..2 twice in block 0: the fold `nu % a.Fin == f`; padded last block"),
    (5, 7, 5, 3, 2, "<- output features straddle blocks (acc carried, closed by `++finQ == a.Fin`); fins 0..2 twice in block 0: the fold `nu % a.Fin == f`; padded last block (3 neurons)"),
    (6, 3, 3, 2, 4, "<- generic kernels with a padded last block: last block 2 neurons, r0 = 4"),
    (7, 5, 5, 3, 4, "REFUSED (40 % 7): 7 -> 7 below. nb = 5, every block starts at another fin, last block 3 neurons"),
    (7, 7, 7, 1, 6, "every block starts at another fin, the last block is ONE neuron (fin 6, fo 6)"),
    (9, 1, 2, 1, 8, "REFUSED (16 % 9): 9 -> 8 below. Fin > 8: fin 8 is first written by block 1, the first-touch rule `(q == f / 8) ? 0.f : old`; last block ONE neuron"),
    (9, 8, 9, 8, 1, "<- Fin > 8: fin 8 is first written by block 1, the first-touch rule `(q == f / 8) ? 0.f : old`; every block starts at another fin"),
    (12, 2, 3, 8, 4, "fins 8..11 first touched by block 1, touched again by block 2"),
    (16, 3, 6, 8, 8, "two blocks per output feature: acc carried over exactly one block boundary, first touch in blocks 0 and 1"),
    (20, 2, 5, 8, 12, "<- fins 16..19 first touched by block 2 (f / 8 == 2), again by block 4"),
    (20, 1, 3, 4, 16, "REFUSED (24 % 20): 20 -> 2 above. fins 16..19 first touched by block 2 (f / 8 == 2), padded"),
]
WIDE = [     # the width limits, on the small cloud
    (4, 100, 50, 8, 0, "<- nb = 50: the last MFMA backward ((50 * 312 + 768) * 4 = 65 472 <= 65 536)"),
    (5, 80, 50, 8, 2, "nb = 50 on the generic kernels"),
    (4, 102, 51, 8, 0, "<- nb = 51: MFMA forward with state records, VALU backward"),
    (5, 81, 51, 5, 0, "REFUSED (408 % 5): 6 -> 67 below. nb = 51 on the generic kernels, padded"),
    (6, 67, 51, 2, 4, "nb = 51 on the generic kernels, padded (the only Fin > 4 with a padded 51st block)"),
    (4, 128, 64, 8, 0, "<- nb = 64 == MCCNN_LDS_MAX_NB: the widest MFMA forward"),
    (8, 64, 64, 8, 0, "nb = 64 on the generic kernels"),
    (1, 400, 50, 8, 0, "<- factored Fin = 1 path, nb = 50: the last f1_backward"),
    (1, 408, 51, 8, 0, "<- factored forward, VALU backward"),
    (1, 512, 64, 8, 0, "<- the widest layer the factored path takes (f1_shape: nb <= 64)"),
    (1, 520, 65, 8, 0, "nb = 65: VALU forward and backward, no state (4 -> 130 in tests/test_gpu_parity.py is the Fin > 1 twin)"),
]
LATTICE = [c + ("A",) for c in STATIC + GENERIC] + [c + ("W",) for c in WIDE]


def accepted(c):
    """the reference's shape rule (spatial_conv.cc:290): the padded neuron count is a multiple of Fin"""
    return (8 * c[2]) % c[0] == 0


def case_id(c):
    return "%dto%d" % (c[0], c[1])


def check_table():
    """the facts the comments state, recomputed"""
    for fin, fout, nb, last, r0, _why, _g in LATTICE:
        assert block_facts(fin, fout) == (nb, last, r0), (fin, fout, block_facts(fin, fout))
        assert accepted((fin, fout, nb)) == (not _why.startswith("REFUSED")), (fin, fout)
        if accepted((fin, fout, nb)) and fin > 1:
            assert (8 * nb - fin * fout) % fin == 0 and (fin <= 7 or last == 8)    # padded by whole output features only
    assert sorted(c[:2] for c in LATTICE if not accepted(c)) == [(3, 5), (3, 10), (3, 11), (5, 1), (5, 3), (5, 81), (7, 5), (9, 1), (20, 1)]
    assert BWD_MFMA_MAX_NB == 50 and (51 * WQ_BWD + 768) * 4 > 64 * 1024


# ------------------------------------------------------------------------------------------------- inputs
def cloud_A():
    """the parity cloud of tests/test_gpu_parity.py::test_spatial_conv_fwd_bwd: (pts, bids, B, radius, scaleInv)"""
    pts, bids = make_cloud(1500, 2, 21, "clustered", True)
    return pts, bids, 2, 0.15, True


def cloud_S():
    """the small twin of A for the CPU comparison with float64 autograd (425 points, 7 055 edges; seed 21 gives 597 points and, with make_mlp(2, 7), a pre-activation at 4.7e-8 of its scale: see tests/test_oracle_combin_cpu.py)"""
    pts, bids = make_cloud(400, 2, 22, "clustered", True)
    return pts, bids, 2, 0.15, True


def cloud_W():
    """the small cloud of the wide layers. Seed 22, not 21: with make_mlp(50, 7) the seed-21 cloud (189 points, 2 649 edges)
    has a layer-2 pre-activation at |pre2| / S2 = 4.0e-10, on which the float32 and the float64 ReLU gate disagree (see
    tests/test_oracle_combin_cpu.py)."""
    pts, bids = make_cloud(150, 2, 22, "clustered", True)
    return pts, bids, 2, 0.3, True


def layer_inputs(n, m, fin, fout):
    """(features of the SORTED points [n, Fin], out-gradient [m, Fout]), both in (-1, 1)"""
    feats = (2 * np.random.default_rng(7).random((n, fin)) - 1).astype(np.float32)
    og = (2 * np.random.default_rng(11).random((m, fout)) - 1).astype(np.float32)
    return feats, og


def pooling_cloud():
    """~900 points (a few of them nobody's neighbour) and 300 pooling centres taken from the points plus far ones (rows without
    an edge at the start, in the middle and at the end): m != n. One cloud, absolute radius 0.2.
    -> (pts, bids, centres, centre batch ids, the generator in the state the callers draw their features from)"""
    pts, _ = make_cloud(1450, 1, 33, "clustered", True)   # (ragged: 885 points)
    rng = np.random.default_rng(3)
    lonely = (-5.0 - 3.0 * rng.random((24, 3))).astype(np.float32)      # points no centre reaches
    pts = np.concatenate([pts[:400], lonely[:12], pts[400:], lonely[12:]]).astype(np.float32)
    bids = np.zeros((len(pts), 1), np.int32)
    far = np.array([[9.0, 9.0, 9.0]], np.float32)
    near = pts[np.sort(rng.choice(np.nonzero(pts[:, 0] > -1.0)[0], 294, replace=False))]
    centres = np.concatenate([far, far + 1, near[:150], far + 2, far + 3, near[150:], far + 4, far + 5]).astype(np.float32)
    cb = np.zeros((len(centres), 1), np.int32)
    return pts, bids, centres, cb, rng


def off(a, nbytes):
    """A contiguous [rows, F] view holding a's values that starts `nbytes` behind a fresh (16-byte aligned) allocation."""
    import torch
    k, r = divmod(nbytes, a.element_size())
    assert r == 0
    buf = torch.empty(a.numel() + 16, dtype=a.dtype, device=a.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + a.numel()].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == nbytes
    return v
