#!/usr/bin/env python3
"""The MCSeg graph of the reference (models/MCSeg.py create_network: a four-level encoder / decoder for per-point part
segmentation) written against mccnn_amd's builder and dense helpers, the way examples/mcclass_s.py writes MCClassS, plus a
synthetic training loop. The layer names, radii, widths and order are the reference's, so the variables carry its names.

Every concatenation that feeds a batch norm + ReLU + dropout block -- six of them -- is handed to batch_norm_RELU_drop_out
as a LIST of its leaf blocks (a nested concatenation as the flattened list): with VariableStore(fused=True, fusedCat=True)
the block then reads the segments where they are (one library op, no torch.cat, one contiguous gradient per segment), and
in every other case the helper concatenates and runs what it ran before.

    python examples/mcseg.py [--steps 20] [--fused-glue] [--fused-cat] [--fused-linear] [--fused-loss] [--fused-adam]
                             [--clip-norm C] [--skip-nonfinite]
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder  # noqa: E402
from mccnn_amd.MCNetworkUtils import (MLP_2_hidden, batch_norm_RELU_drop_out, conv_1x1, conv_1x1_batch_norm_RELU_drop_out,  # noqa: E402
                                      VariableStore, part_iou, segmentation_counts, voxel_counts, voxel_scores)
from mcclass_s import NUM_PARTS, make_optimizer, part_labels, synthetic_normals_batch  # noqa: E402


class MCSeg(torch.nn.Module):
    """models/MCSeg.py create_network(): 3 Poisson levels under the input, an encoder of four convolutions with three
    poolings, a decoder of three up-samplings with skip connections, and the per-point MLP over the features and the one-hot
    category of the point's cloud. A torch.nn.Module as MCClassS is: `parameters()` / `state_dict()` see every variable under
    the reference's name."""

    RADII = [0.025, 0.1, 0.4]
    #: the batch-norm blocks of the graph: 20 around the convolutions, 2 in the MLP (no initial one: useInitBN=False)
    NUM_BN_BLOCKS = 22

    def __init__(self, numInputFeatures, batchSize, k, numCats, numParts, device, ops=None, fused=False, fusedCat=False,
                 fusedLinear=False, fusedLoss=False, rows=None):
        super().__init__()
        self.args = (numInputFeatures, batchSize, k, numCats, numParts)
        # fused: batch norm + ReLU + dropout of a glue block as one library op (VariableStore.fused_)
        # fusedCat: with fused, the blocks over a concatenation read its segments in place (VariableStore.fusedCat_)
        # fusedLinear: the six conv_1x1 + ..._Out_BN pairs as one library op each. The pairs only: the store's own switch stays
        #       as the caller leaves it (off here), so the hidden layers of the per-point MLP remain a matmul followed by the
        #       glue block. Their biases have an exactly zero gradient (a batch norm follows), and over the N rows of a
        #       segmentation batch the fused op's cancelling column sum for it is ten times torch's rounding (2.1e-7 beside
        #       2.2e-8 at 4096 rows); whoever wants them fused as well sets net.store.fusedLinear_ = True
        # fusedLoss: with labels handed to forward(), the last linear of the MLP and the softmax cross-entropy as one library op
        # rows: torch.bfloat16 keeps the input rows of the depth-wise layers behind a single-tensor block in bf16 (the block is
        #       the cast); None: every call is the f32 network's
        self.fusedLinear = bool(fusedLinear)
        self.rows = rows
        self.store = VariableStore(device, fused=fused, fusedCat=fusedCat, fusedLoss=fusedLoss)
        self.ops = ops  # None = the HIP op surface; the parity tests pass the CPU checker's
        self.convBuilder = ConvolutionBuilder(KDEWindow=0.25, device=device, ops=ops)

    def prefetch_hierarchy(self, points, batchIds, after=None):
        """Starts the point hierarchy of a batch on a stream of its own (MCClassS.prefetch_hierarchy)."""
        return PointHierarchy.prefetch(points, batchIds, self.RADII, self.args[1], after=after)

    def hierarchy(self, points, batchIds, features, prefetched=None):
        """The network's point hierarchy for a batch (prefetched: what prefetch_hierarchy() returned for it)."""
        return PointHierarchy(points, features, batchIds, self.RADII, "MCSeg_PH", self.args[1], ops=self.ops, prefetched=prefetched)

    def forward(self, points, batchIds, features, catLabels, isTraining, keepProbConv=1.0, keepProbFull=0.5, useConvDropOut=False,
                useDropOutFull=True, prefetched=None, hierarchy=None, nextHierarchy=None, labels=None):
        """catLabels: the category of every point's cloud, integer (N,) or (N, 1). labels: one part label per point -- the
        result is then the LossHead of MLP_2_hidden over the last linear instead of the (N, numParts) logits. hierarchy /
        nextHierarchy: as in MCClassS.forward."""
        numInputFeatures, batchSize, k, numCats, numParts = self.args
        st, cb = self.store, self.convBuilder
        cb.reset()
        if nextHierarchy is not None:
            cb.prefetch_step(nextHierarchy)
        ph = hierarchy if hierarchy is not None else self.hierarchy(points, batchIds, features, prefetched)
        toRows = {} if self.rows is None else {"outDtype": self.rows}          # into a depth-wise layer
        toDense = {} if self.rows is None else {"outDtype": torch.float32}     # into a matmul

        def glue(name, x, **kw):   # x: a tensor, or the list of blocks whose concatenation it stands for
            return batch_norm_RELU_drop_out(name, x, isTraining, useConvDropOut, keepProbConv, st, **kw)

        def reduce(name, x, numIn, numOut):   # conv_1x1(name) + name_Out_BN, into a depth-wise layer
            if self.fusedLinear:
                was, st.fusedLinear_ = st.fusedLinear_, True     # (for this pair; the MLP below sees the store's own setting)
                try:
                    return conv_1x1_batch_norm_RELU_drop_out(name, name + "_Out_BN", x, numIn, numOut, isTraining, useConvDropOut,
                                                             keepProbConv, st, **toRows)
                finally:
                    st.fusedLinear_ = was
            return glue(name + "_Out_BN", conv_1x1(name, x, numIn, numOut, st), **toRows)

        def conv(name, level, x, numIn, radius, **kw):
            return cb.create_convolution(convName=name, inPointHierarchy=ph, inPointLevel=level, inFeatures=x, inNumFeatures=numIn,
                                         convRadius=radius, **kw)

        # ---- encoder
        convFeatures1 = conv("Conv_1", 0, features, numInputFeatures, 0.03, outNumFeatures=k, multiFeatureConv=True)
        bn = glue("Reduce_Pool_1_In_BN", convFeatures1, **toDense)
        bn = reduce("Reduce_Pool_1", bn, k, k * 2)
        poolFeatures1 = conv("Pool_1", 0, bn, k * 2, 0.05, outPointLevel=1, KDEWindow=0.2)

        bn = glue("Conv_2_In_BN", poolFeatures1, **toRows)
        convFeatures2 = [poolFeatures1, conv("Conv_2", 1, bn, k * 2, 0.1)]                       # tf.concat, k * 4 wide
        bn = glue("Reduce_Pool_2_In_BN", convFeatures2, **toDense)
        bn = reduce("Reduce_Pool_2", bn, k * 4, k * 4)
        poolFeatures2 = conv("Pool_2", 1, bn, k * 4, 0.2, outPointLevel=2, KDEWindow=0.2)

        bn = glue("Conv_3_In_BN", poolFeatures2, **toRows)
        convFeatures3 = [poolFeatures2, conv("Conv_3", 2, bn, k * 4, 0.4)]                       # k * 8 wide
        bn = glue("Reduce_Pool_3_In_BN", convFeatures3, **toDense)
        bn = reduce("Reduce_Pool_3", bn, k * 8, k * 8)
        poolFeatures3 = conv("Pool_3", 2, bn, k * 8, 0.8, outPointLevel=3, KDEWindow=0.2)

        bn = glue("Conv_4_In_BN", poolFeatures3, **toRows)
        convFeatures4 = [poolFeatures3, conv("Conv_4", 3, bn, k * 8, math.sqrt(3.0) + 0.1)]      # k * 16 wide

        # ---- decoder
        bn = glue("Up_3_4_BN", convFeatures4, **toRows)
        upFeatures3_4 = conv("Up_3_4", 3, bn, k * 16, math.sqrt(3.0) + 0.1, outPointLevel=2)
        bn = glue("DeConv_3_Reduce_In_BN", [upFeatures3_4] + convFeatures3, **toDense)           # k * 24 wide, three blocks
        bn = reduce("DeConv_3_Reduce", bn, k * 24, k * 8)
        deConvFeatures3 = conv("DeConv_3", 2, bn, k * 8, 0.4)

        bn = glue("Up_2_3_BN", deConvFeatures3, **toRows)
        upFeatures2_3 = conv("Up_2_3", 2, bn, k * 8, 0.2, outPointLevel=1)
        bn = glue("DeConv_2_Reduce_In_BN", [upFeatures2_3] + convFeatures2, **toDense)           # k * 12 wide
        bn = reduce("DeConv_2_Reduce", bn, k * 12, k * 4)
        deConvFeatures2 = conv("DeConv_2", 1, bn, k * 4, 0.1)

        bn = glue("Up_1_2_BN", deConvFeatures2, **toRows)
        upFeatures1_2 = conv("Up_1_2", 1, bn, k * 4, 0.05, outPointLevel=0)
        bn = glue("Up_1_3_BN", deConvFeatures3, **toRows)
        upFeatures1_3 = conv("Up_1_3", 2, bn, k * 8, 0.2, outPointLevel=0)
        bn = glue("DeConv_1_Reduce_In_BN", [upFeatures1_2, upFeatures1_3, convFeatures1], **toDense)   # k * 13 wide
        bn = reduce("DeConv_1_Reduce", bn, k * 13, k * 4)
        deConvFeatures1 = conv("DeConv_1", 0, bn, k * 4, 0.03)

        # ---- the per-point MLP over the features and the one-hot category (a torch.cat: it feeds a linear layer)
        finalInput = glue("BNRELUDROP_hier_final", deConvFeatures1, **toDense)
        oneHot = torch.nn.functional.one_hot(catLabels.reshape(-1).long(), numCats).to(finalInput.dtype)
        finalInput = torch.cat([oneHot, finalInput], 1)
        out = MLP_2_hidden(finalInput, k * 4 + numCats, k * 4, k * 2, numParts, "Final_Logits", keepProbFull, isTraining, useDropOutFull,
                           useInitBN=False, store=st, labels=labels)
        self.lastHierarchy = ph
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--fused-glue", action="store_true", help="the glue blocks as one library op each (VariableStore(fused=True))")
    ap.add_argument("--fused-cat", action="store_true",
                    help="with --fused-glue: the blocks over a concatenation read its segments in place (VariableStore(fusedCat=True))")
    ap.add_argument("--bf16-rows", action="store_true",
                    help="bf16 input rows for the depth-wise layers (MCSeg(rows=torch.bfloat16)); the blocks over a concatenation "
                         "then see bf16 and mixed-type segments")
    ap.add_argument("--fused-linear", action="store_true", help="the six conv_1x1 + ..._Out_BN pairs as one library op each")
    ap.add_argument("--fused-loss", action="store_true",
                    help="the last linear of the MLP + softmax cross-entropy as one library op; part IoU and voxel accuracy from "
                         "device counts")
    ap.add_argument("--fused-adam", action="store_true", help="the optimiser step as one library op (mccnn_amd.optim.FusedAdam)")
    ap.add_argument("--weight-decay", type=float, default=0.0, metavar="C", help="with --fused-adam: L2 decay")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="C", help="with --fused-adam: clip to the global gradient norm C")
    ap.add_argument("--skip-nonfinite", action="store_true", help="with --fused-adam: leave out a step with a non-finite gradient norm")
    args = ap.parse_args()
    if args.weight_decay and not args.fused_adam:
        ap.error("--weight-decay needs --fused-adam")
    if (args.clip_norm is not None or args.skip_nonfinite) and not args.fused_adam:
        ap.error("--clip-norm and --skip-nonfinite need --fused-adam")
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    torch.autograd.set_multithreading_enabled(False)   # (one process per GPU: see examples/mcclass_s.py)
    numCats = 4
    net = MCSeg(1, args.batch, args.k, numCats, NUM_PARTS, device, fused=args.fused_glue, fusedCat=args.fused_cat,
                fusedLinear=args.fused_linear, fusedLoss=args.fused_loss, rows=torch.bfloat16 if args.bf16_rows else None)

    def batch():
        P, Bi, F, N = synthetic_normals_batch(args.batch, args.points, rng, device)
        return P, Bi, F, (Bi % numCats).reshape(-1), part_labels(N)

    P, Bi, F, cats, y = batch()
    with torch.no_grad():
        net(P, Bi, F, cats, True)  # creates the variables
    opt = make_optimizer(net, args)
    mask = torch.ones((args.batch, NUM_PARTS), dtype=torch.bool, device=device)   # every cloud has all eight parts
    counts = torch.zeros((args.batch, NUM_PARTS, 3), dtype=torch.int64, device=device)
    voxels = torch.zeros((args.batch, NUM_PARTS, 2), dtype=torch.int64, device=device)
    for step in range(args.steps):
        P, Bi, F, cats, y = batch()
        out = net(P, Bi, F, cats, True, labels=y if args.fused_loss else None)
        loss = out.loss if args.fused_loss else torch.nn.functional.cross_entropy(out, y.long())
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        pred = out if args.fused_loss else out.detach().argmax(1).to(torch.int32)
        segmentation_counts(pred, y, NUM_PARTS, Bi, args.batch, out=counts, store=net.store)
        voxel_counts(P, pred, y, NUM_PARTS, Bi, args.batch, out=voxels, store=net.store)
        if step % 5 == 0 or step == args.steps - 1:
            line = torch.stack([loss.detach().double(), part_iou(counts, mask).mean(), voxel_scores(voxels).meanAcc])
            lossv, iou, vox = line.tolist()   # (the one read-back of this print)
            print("step %3d  loss %.4f  part IoU %.3f  voxel acc %.3f  level sizes %s" % (
                step, lossv, iou, vox, [int(p.shape[0]) for p in net.lastHierarchy.points_]))
            counts.zero_()
            voxels.zero_()


if __name__ == "__main__":
    main()
