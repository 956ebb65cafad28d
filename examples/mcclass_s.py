#!/usr/bin/env python3
"""End-to-end consumer of the drop-in path: the MCClassS and MCNormS graphs of the reference
(models/MCClassS.py:25-77, models/MCNormS.py:25-58) written against mccnn_amd's builder and dense helpers, plus a
tiny synthetic training loop. The graph builders keep the reference's structure line by line; only `tf.` is gone.

    python examples/mcclass_s.py [--steps 20] [--device-loader]
    python examples/mcclass_s.py --normals [--fused-glue] [--fused-loss]     # MCNormS on the ellipsoids' analytic normals
    python examples/mcclass_s.py --parts [--fused-glue] [--fused-loss]       # per-point part labels, part IoU from device counts
    python examples/mcclass_s.py --fused-adam [--weight-decay 1e-4]          # the optimiser step as one library op (any mode)
    python examples/mcclass_s.py --fused-adam --clip-norm 1.0 --skip-nonfinite   # ... clipped by the global gradient norm, inside the op

--device-loader builds the batches on the GPU (mccnn_amd.device_batcher.DeviceBatcher: a pool of synthetic models uploaded
once, non-uniform sampling and rotation per batch on the device) instead of uploading host arrays.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mccnn_amd.MCConvBuilder import PointHierarchy, ConvolutionBuilder
from mccnn_amd.MCNetworkUtils import (MLP_2_hidden, batch_norm_RELU_drop_out, conv_1x1, conv_1x1_batch_norm_RELU_drop_out,
                                      VariableStore, conv_1x1_softmax_cross_entropy, cosine_distance_loss, mean_angle, part_iou,
                                      segmentation_counts, voxel_counts, voxel_scores)


class MCClassS(torch.nn.Module):
    """models/MCClassS.py create_network(): 3 Poisson levels, 3 MC convolutions, global-feature MLP. A torch.nn.Module
    whose sub-modules (the convolution builder and the dense helpers' variable store) register every variable under
    the reference's name, so `parameters()` / `state_dict()` / optimisers / DDP see the whole network."""

    def __init__(self, numInputFeatures, batchSize, k, numOutCat, device, ops=None, fused=False, rows=None, fusedLinear=False,
                 fusedSync=False, fusedLoss=False):
        super().__init__()
        self.args = (numInputFeatures, batchSize, k, numOutCat)
        # rows (extension): torch.bfloat16 keeps the input rows of the depth-wise Conv_2 and Conv_3 in bf16 (they gather
        # half the bytes). The glue blocks around them are the casts -- with fused=True one library op each, f32 statistics
        # either way; the 1x1 matmuls and the MLP stay f32. None: every call is the f32 network's.
        self.rows = rows
        # fused (extension): batch norm + ReLU + dropout of the dense glue as one library op (VariableStore.fused_)
        # fusedLinear (extension): Reduce_k + Reduce_k_Out_BN and the hidden layers of the MLP as one library op each
        # (VariableStore.fusedLinear_, conv_1x1_batch_norm_RELU_drop_out)
        self.fusedLinear = bool(fusedLinear)
        # fusedSync (extension): with fused, the glue stays a library op when its statistics run across ranks
        # (VariableStore.fusedSync_)
        # fusedLoss (extension): with labels handed to forward(), the last linear of the MLP and the softmax cross-entropy
        # behind it as one library op (VariableStore.fusedLoss_)
        self.store = VariableStore(device, fused=fused, fusedLinear=fusedLinear, fusedSync=fusedSync, fusedLoss=fusedLoss)
        self.ops = ops  # None = the HIP op surface; the parity tests pass the CPU checker's
        self.convBuilder = ConvolutionBuilder(KDEWindow=0.2, device=device, ops=ops)

    RADII = [0.1, 0.4, math.sqrt(3.0) + 0.1]

    def prefetch_hierarchy(self, points, batchIds, after=None):
        """Extension: starts the point hierarchy of a batch on a stream of its own (PointHierarchy.prefetch) -- call it for
        batch k + 1 before the forward pass of batch k and hand the result to forward(prefetched=...). after: what the
        build waits for -- None: the calling stream (the batch was uploaded there), a torch.cuda.Event of the loader's
        upload stream, or True (the batch is complete)."""
        return PointHierarchy.prefetch(points, batchIds, self.RADII, self.args[1], after=after)

    def hierarchy(self, points, batchIds, features, prefetched=None):
        """The network's point hierarchy for a batch (prefetched: what prefetch_hierarchy() returned for it)."""
        return PointHierarchy(points, features, batchIds, self.RADII, "MCClassS_PH", self.args[1], ops=self.ops,
                              prefetched=prefetched)

    def forward(self, points, batchIds, features, isTraining, keepProbConv=1.0, keepProbFull=0.5, useConvDropOut=False,
                 useDropOutFull=True, prefetched=None, hierarchy=None, nextHierarchy=None, labels=None):
        """labels (extension): one class per cloud -- the result is then the LossHead of MLP_2_hidden (loss, predictions, count of
        correct rows, denominator) over the last linear instead of the logits; None: the logits, every call as before.
        hierarchy (extension): this batch's hierarchy, built a step ago with self.hierarchy(); nextHierarchy: the NEXT
        batch's -- its grids, neighbour lists, PDFs and row plans are then started under this batch's layers
        (ConvolutionBuilder.prefetch_step) and the next forward pass finds them built."""
        numInputFeatures, batchSize, k, numOutCat = self.args
        st, mConvBuilder = self.store, self.convBuilder
        mConvBuilder.reset()
        if nextHierarchy is not None:
            mConvBuilder.prefetch_step(nextHierarchy)
        mPointHierarchy = hierarchy if hierarchy is not None else self.hierarchy(points, batchIds, features, prefetched)
        convFeatures1 = mConvBuilder.create_convolution(
            convName="Conv_1", inPointHierarchy=mPointHierarchy, inPointLevel=0, outPointLevel=1, inFeatures=features,
            inNumFeatures=numInputFeatures, outNumFeatures=k, convRadius=0.2, multiFeatureConv=True)
        convFeatures1 = batch_norm_RELU_drop_out("Reduce_1_In_BN", convFeatures1, isTraining, useConvDropOut, keepProbConv, st)
        toRows = {} if self.rows is None else {"outDtype": self.rows}          # into a depth-wise layer
        toDense = {} if self.rows is None else {"outDtype": torch.float32}     # out of one, into a matmul
        if self.fusedLinear:
            convFeatures1 = conv_1x1_batch_norm_RELU_drop_out("Reduce_1", "Reduce_1_Out_BN", convFeatures1, k, k * 2, isTraining,
                                                              useConvDropOut, keepProbConv, st, **toRows)
        else:
            convFeatures1 = conv_1x1("Reduce_1", convFeatures1, k, k * 2, st)
            convFeatures1 = batch_norm_RELU_drop_out("Reduce_1_Out_BN", convFeatures1, isTraining, useConvDropOut, keepProbConv,
                                                     st, **toRows)
        convFeatures2 = mConvBuilder.create_convolution(
            convName="Conv_2", inPointHierarchy=mPointHierarchy, inPointLevel=1, outPointLevel=2,
            inFeatures=convFeatures1, inNumFeatures=k * 2, convRadius=0.8)
        convFeatures2 = batch_norm_RELU_drop_out("Reduce_2_In_BN", convFeatures2, isTraining, useConvDropOut, keepProbConv, st,
                                                 **toDense)
        if self.fusedLinear:
            convFeatures2 = conv_1x1_batch_norm_RELU_drop_out("Reduce_2", "Reduce_2_Out_BN", convFeatures2, k * 2, k * 4, isTraining,
                                                              useConvDropOut, keepProbConv, st, **toRows)
        else:
            convFeatures2 = conv_1x1("Reduce_2", convFeatures2, k * 2, k * 4, st)
            convFeatures2 = batch_norm_RELU_drop_out("Reduce_2_Out_BN", convFeatures2, isTraining, useConvDropOut, keepProbConv,
                                                     st, **toRows)
        convFeatures3 = mConvBuilder.create_convolution(
            convName="Conv_3", inPointHierarchy=mPointHierarchy, inPointLevel=2, outPointLevel=3,
            inFeatures=convFeatures2, inNumFeatures=k * 4, convRadius=math.sqrt(3.0) + 0.1)
        finalInput = batch_norm_RELU_drop_out("BNRELUDROP_final", convFeatures3, isTraining, useConvDropOut, keepProbConv, st,
                                              **toDense)
        finalLogits = MLP_2_hidden(finalInput, k * 4, k * 2, k, numOutCat, "Final_Logits", keepProbFull, isTraining,
                                   useDropOutFull, store=st, labels=labels)
        self.lastHierarchy = mPointHierarchy
        return finalLogits


class MCNormS(torch.nn.Module):
    """models/MCNormS.py create_network(): two same-level multi-feature convolutions (normal estimation)."""

    def __init__(self, numInputFeatures, batchSize, k, device, ops=None, fused=False, fusedSync=False, fusedLoss=False,
                 outFeatures=3):
        super().__init__()
        self.args = (numInputFeatures, batchSize, k)
        # outFeatures (extension): the width of the second convolution -- 3, the normal, in the reference; wider for the
        # per-point features of forward(partLabels=...)
        self.outFeatures = int(outFeatures)
        # fusedLoss (extension): with normals handed to forward(), the cosine-distance loss and its metrics as one library op
        # (VariableStore.fusedLoss_, cosine_distance_loss)
        self.store = VariableStore(device, fused=fused, fusedSync=fusedSync, fusedLoss=fusedLoss)
        self.ops = ops
        self.convBuilder = ConvolutionBuilder(KDEWindow=0.2, device=device, ops=ops)

    def hierarchy(self, points, batchIds, features):
        """The network's point hierarchy for a batch (the input level only)."""
        return PointHierarchy(points, features, batchIds, [], "MCNormS_PH", self.args[1], ops=self.ops)

    def forward(self, points, batchIds, features, isTraining, normals=None, normalWeights=None, hierarchy=None,
                nextHierarchy=None, partLabels=None, numParts=None):
        """normals (extension): the [N, 3] target normals -- the result is then the NormalHead of cosine_distance_loss (loss,
        sum of cosines, sum of angles, denominator) over the last convolution's output, normalWeights its row weights; None:
        the [N, 3] prediction, every call as before. partLabels (extension): one part label per point -- the second
        convolution's output (outFeatures wide) is then the per-point feature of a segmentation head, batch norm + ReLU and
        conv_1x1_softmax_cross_entropy over numParts classes, and the result is its LossHead. hierarchy / nextHierarchy
        (extension): as in MCClassS.forward."""
        numInputFeatures, batchSize, k = self.args
        cb = self.convBuilder
        cb.reset()
        if nextHierarchy is not None:
            cb.prefetch_step(nextHierarchy)
        ph = hierarchy if hierarchy is not None else self.hierarchy(points, batchIds, features)
        c1 = cb.create_convolution(convName="Conv_1", inPointHierarchy=ph, inPointLevel=0, inFeatures=features,
                                   inNumFeatures=numInputFeatures, outNumFeatures=k, convRadius=0.15, multiFeatureConv=True)
        c1 = batch_norm_RELU_drop_out("BN_RELU", c1, isTraining, False, False, self.store)
        pred = cb.create_convolution(convName="Conv_2", inPointHierarchy=ph, inPointLevel=0, inFeatures=c1,
                                     inNumFeatures=k, outNumFeatures=self.outFeatures, convRadius=0.15, multiFeatureConv=True)
        if partLabels is not None:
            feats = batch_norm_RELU_drop_out("Parts_BN_RELU", pred, isTraining, False, False, self.store)
            return conv_1x1_softmax_cross_entropy("Parts_Logits", feats, self.outFeatures, numParts, partLabels, store=self.store)
        if normals is None:
            return pred
        return cosine_distance_loss(pred, normals, normalWeights, store=self.store)


def synthetic_normals_batch(batchSize, nPts, rng, device):
    """Ellipsoids as in synthetic_batch with their analytic normals: n is proportional to p / axes^2 in the unscaled frame
    (the gradient of sum (p_j / axes_j)^2), and the unit-box normalisation, a translation and one scale, leaves it as it is.
    -> (points, batch ids, features, normals)."""
    pts, bids, nrm = [], [], []
    for b in range(batchSize):
        axes = np.array([1.0, rng.uniform(0.3, 1.0), rng.uniform(0.3, 1.0)])
        v = rng.normal(size=(nPts, 3))
        p = v / np.linalg.norm(v, axis=1, keepdims=True) * axes
        g = p / (axes * axes)
        nrm.append((g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32))
        p = (p - p.min(0)) / (p.max(0) - p.min(0)).max()
        pts.append(p.astype(np.float32))
        bids.append(np.full((nPts, 1), b, np.int32))
    t = lambda a: torch.from_numpy(a).to(device)
    P, Bi = t(np.concatenate(pts)), t(np.concatenate(bids))
    return P, Bi, torch.ones((P.shape[0], 1), dtype=torch.float32, device=device), t(np.concatenate(nrm))


def make_optimizer(net, args, lr=5e-3):
    """The optimiser of all three training loops. Default: torch.optim.Adam, as before. --fused-adam: mccnn_amd.optim.FusedAdam,
    the step as one library op, with the reference's L2 term (ModelNet.py:33-56: l2_regularizer over the 'weight_decay_loss'
    collection, added to the loss) as --weight-decay C over the two collections of the network. --clip-norm C and
    --skip-nonfinite (both with --fused-adam): the gradients clipped to the global norm C, and a step with a non-finite norm
    left out, both inside the op (FusedAdam(maxGradNorm, skipNonFinite))."""
    clip, skip = getattr(args, "clip_norm", None), bool(getattr(args, "skip_nonfinite", False))
    if not args.fused_adam:
        if clip is not None or skip:
            raise ValueError("--clip-norm and --skip-nonfinite need --fused-adam")
        return torch.optim.Adam(net.parameters(), lr=lr)
    from mccnn_amd.optim import FusedAdam
    decay = net.store.get_collection('weight_decay_loss') + net.convBuilder.get_collection('weight_decay_loss')
    return FusedAdam(net.parameters(), lr=lr, weightDecay=args.weight_decay, decayParams=decay, maxGradNorm=clip, skipNonFinite=skip)


def train_normals(args, device, rng):
    """--normals: MCNormS on the synthetic ellipsoids, the loss and the mean angle from the NormalHead of the model."""
    net = MCNormS(1, args.batch, 16, device, fused=args.fused_glue, fusedLoss=args.fused_loss)
    P, Bi, F, N = synthetic_normals_batch(args.batch, args.points, rng, device)
    net(P, Bi, F, True)  # creates the variables
    opt = make_optimizer(net, args)
    for step in range(args.steps):
        P, Bi, F, N = synthetic_normals_batch(args.batch, args.points, rng, device)
        head = net(P, Bi, F, True, normals=N)
        opt.zero_grad(set_to_none=True)
        head.loss.backward()
        opt.step()
        if step % 5 == 0 or step == args.steps - 1:
            print("step %3d  loss %.4f  mean angle %.2f deg" % (step, float(head.loss), math.degrees(float(mean_angle(head)))))


NUM_PARTS = 8


def part_labels(normals):
    """The part of a point as a pure function of its analytic normal: the octant of the normal, 8 parts (int32 [N])."""
    s = (normals >= 0).to(torch.int32)
    return s[:, 0] + 2 * s[:, 1] + 4 * s[:, 2]


def train_parts(args, device, rng):
    """--parts: a per-point network (MCNormS's two convolutions, 16 features wide, and a softmax cross-entropy head) on the
    synthetic ellipsoids with the octant of the normal as part label. The counts behind the part IoU are accumulated on the
    device over the steps between two prints (segmentation_counts into one tensor), and beside them the counts behind the
    voxel accuracy (voxel_counts: 5 cm voxels over every cloud's own box, majority votes per voxel); a print reads back the
    loss, the accuracy, the mean of part_iou over the clouds seen since the last one and the voxel accuracy (voxel_scores) in
    ONE transfer -- nothing is read back per step (with --fused-loss; without it voxel_counts runs its torch code, whose
    torch.unique waits for the device)."""
    net = MCNormS(1, args.batch, 16, device, fused=args.fused_glue, fusedLoss=args.fused_loss, outFeatures=16)
    P, Bi, F, N = synthetic_normals_batch(args.batch, args.points, rng, device)
    net(P, Bi, F, True, partLabels=part_labels(N), numParts=NUM_PARTS)  # creates the variables
    opt = make_optimizer(net, args)
    mask = torch.ones((args.batch, NUM_PARTS), dtype=torch.bool, device=device)   # every cloud has all eight parts
    counts = torch.zeros((args.batch, NUM_PARTS, 3), dtype=torch.int64, device=device)
    voxels = torch.zeros((args.batch, NUM_PARTS, 2), dtype=torch.int64, device=device)
    for step in range(args.steps):
        P, Bi, F, N = synthetic_normals_batch(args.batch, args.points, rng, device)
        y = part_labels(N)
        head = net(P, Bi, F, True, partLabels=y, numParts=NUM_PARTS)
        opt.zero_grad(set_to_none=True)
        head.loss.backward()
        opt.step()
        segmentation_counts(head, y, NUM_PARTS, Bi, args.batch, out=counts, store=net.store)
        voxel_counts(P, head, y, NUM_PARTS, Bi, args.batch, out=voxels, store=net.store)
        if step % 5 == 0 or step == args.steps - 1:
            line = torch.stack([head.loss.detach().double(), head.correct.double() / head.denom.double(), part_iou(counts, mask).mean(),
                                voxel_scores(voxels).meanAcc])
            loss, acc, iou, vox = line.tolist()   # (the one read-back of this print)
            print("step %3d  loss %.4f  acc %.2f  part IoU %.3f  voxel acc %.3f" % (step, loss, acc, iou, vox))
            counts.zero_()
            voxels.zero_()


def synthetic_batch(batchSize, nPts, numCat, rng, device):
    """Shapes whose class is a geometric property: ellipsoids with class-dependent axis ratios, unit-box normalised."""
    pts, bids, labels = [], [], []
    for b in range(batchSize):
        c = int(rng.integers(0, numCat))
        axes = np.array([1.0, 0.3 + 0.7 * c / max(numCat - 1, 1), 0.3 + 0.7 * ((c * 3) % numCat) / max(numCat - 1, 1)])
        v = rng.normal(size=(nPts, 3))
        p = v / np.linalg.norm(v, axis=1, keepdims=True) * axes
        p = (p - p.min(0)) / (p.max(0) - p.min(0)).max()
        pts.append(p.astype(np.float32))
        bids.append(np.full((nPts, 1), b, np.int32))
        labels.append(c)
    t = lambda a: torch.from_numpy(a).to(device)
    P, Bi = t(np.concatenate(pts)), t(np.concatenate(bids))
    return P, Bi, torch.ones((P.shape[0], 1), dtype=torch.float32, device=device), t(np.array(labels, np.int64))


def device_loader(batchSize, nPts, numCat, rng, device, batchesPerEpoch=8):
    """-> a function returning (points, batch ids, features, labels) like synthetic_batch, from a DeviceBatcher over a pool of
    batchesPerEpoch * batchSize ellipsoids (every batch is full) of 4 * nPts points with normals: uniform, split, gradient
    and lambert sampling, random rotations about the y axis. check=False: nothing is read back, the host only plans."""
    from mccnn_amd.device_batcher import DeviceBatcher
    models, cats = [], []
    for _ in range(batchesPerEpoch * batchSize):
        c = int(rng.integers(0, numCat))
        axes = np.array([1.0, 0.3 + 0.7 * c / max(numCat - 1, 1), 0.3 + 0.7 * ((c * 3) % numCat) / max(numCat - 1, 1)])
        v = rng.normal(size=(4 * nPts, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        p = v * axes
        models.append({"pts": (p - p.min(0)) / (p.max(0) - p.min(0)).max(), "normals": v})
        cats.append(c)
    db = DeviceBatcher(models, nPts, 0.8, batchSize, [0, 1, 2, 3], categories=cats, augment=True, seed=0, device=device)

    def batch():
        if not db.has_more_batches():
            db.start_iteration()
        _, P, Bi, F, _, y, _, _ = db.get_next_batch(check=False)
        return P, Bi, F, y
    return batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-loader", action="store_true", help="build the batches on the GPU (DeviceBatcher)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--fused-glue", action="store_true",
                    help="batch norm + ReLU + dropout of the dense layers as one library op (VariableStore(fused=True))")
    ap.add_argument("--fused-linear", action="store_true",
                    help="Reduce_k + Reduce_k_Out_BN and the hidden layers of the MLP as one library op each "
                         "(VariableStore(fusedLinear=True))")
    ap.add_argument("--fused-loss", action="store_true",
                    help="the last linear of the MLP + softmax cross-entropy + arg-max as one library op "
                         "(VariableStore(fusedLoss=True)); the loop then takes the loss and the accuracy from its LossHead. "
                         "With --normals: the cosine-distance loss and its metrics as one library op")
    ap.add_argument("--normals", action="store_true",
                    help="train MCNormS (normal estimation) on the ellipsoids' analytic normals instead of MCClassS")
    ap.add_argument("--parts", action="store_true",
                    help="train a per-point part segmentation (the octant of the normal, 8 parts) and print the part IoU from "
                         "counts kept on the device (segmentation_counts, part_iou), and the voxel accuracy beside it "
                         "(voxel_counts, voxel_scores)")
    ap.add_argument("--bf16-rows", action="store_true",
                    help="keep the input rows of the depth-wise convolutions in bfloat16 (MCClassS(rows=torch.bfloat16))")
    ap.add_argument("--fused-adam", action="store_true",
                    help="the optimiser step as one library op (mccnn_amd.optim.FusedAdam) instead of torch.optim.Adam")
    ap.add_argument("--weight-decay", type=float, default=0.0, metavar="C",
                    help="with --fused-adam: L2 decay C over the 'weight_decay_loss' collections (the reference's "
                         "l2_regularizer(scale=C) term)")
    ap.add_argument("--clip-norm", type=float, default=None, metavar="C",
                    help="with --fused-adam: clip the gradients to the global norm C inside the optimiser op")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="with --fused-adam: a step whose gradient norm is inf or NaN changes nothing")
    args = ap.parse_args()
    if args.weight_decay and not args.fused_adam:
        ap.error("--weight-decay needs --fused-adam")
    if (args.clip_norm is not None or args.skip_nonfinite) and not args.fused_adam:
        ap.error("--clip-norm and --skip-nonfinite need --fused-adam")
    device = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    # one process per GPU: run the backward pass on the calling thread -- the autograd engine's per-device worker thread
    # only adds a hand-off per backward() and this network is host-bound (cfg1 step: 4.0 -> 3.3 ms, tools/e2e_time.py)
    torch.autograd.set_multithreading_enabled(False)
    if args.normals:
        return train_normals(args, device, rng)
    if args.parts:
        return train_parts(args, device, rng)
    net = MCClassS(1, args.batch, 16, 4, device, fused=args.fused_glue, rows=torch.bfloat16 if args.bf16_rows else None,
                   fusedLinear=args.fused_linear, fusedLoss=args.fused_loss)
    make_batch = device_loader(args.batch, args.points, 4, rng, device) if args.device_loader else \
        (lambda: synthetic_batch(args.batch, args.points, 4, rng, device))
    P, Bi, F, y = make_batch()
    net(P, Bi, F, True)  # creates the variables
    opt = make_optimizer(net, args)
    # the loader runs two batches ahead: the hierarchy of batch k + 2 is requested (helper thread, own stream) while batch
    # k trains; the one of batch k + 1 is complete by then, and its geometry is started under batch k's layers
    cur = make_batch()
    nxt = make_batch()
    ph_cur = net.hierarchy(cur[0], cur[1], cur[2])
    fut_nxt = net.prefetch_hierarchy(nxt[0], nxt[1])
    for step in range(args.steps):
        P, Bi, F, y = cur
        ph_nxt = net.hierarchy(nxt[0], nxt[1], nxt[2], prefetched=fut_nxt)
        after = make_batch()
        fut_after = net.prefetch_hierarchy(after[0], after[1])
        out = net(P, Bi, F, True, hierarchy=ph_cur, nextHierarchy=ph_nxt, labels=y if args.fused_loss else None)
        cur, nxt, ph_cur, fut_nxt = nxt, after, ph_nxt, fut_after
        loss = out.loss if args.fused_loss else torch.nn.functional.cross_entropy(out, y)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        if step % 5 == 0 or step == args.steps - 1:
            acc = float(out.correct) / float(out.denom) if args.fused_loss else float((out.argmax(1) == y).float().mean())
            print("step %3d  loss %.4f  acc %.2f  level sizes %s" % (
                step, float(loss), acc, [int(p.shape[0]) for p in net.lastHierarchy.points_]))


if __name__ == "__main__":
    main()
