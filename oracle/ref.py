"""ctypes/NumPy front-end of oracle/_ref/libmccnn_ref.so: the REFERENCE's own kernels, compiled with hipcc for gfx950
by oracle/ref_build.py, run on the GPU.

TEST INFRASTRUCTURE ONLY. `Reference` has the method names and argument orders of `oracle.Oracle`, NumPy in and NumPy
out, so a test reads run_chain(reference, ...) like run_chain(oracle, ...). What each method does is the call sequence
of the reference's TensorFlow op wrapper (tf_ops/*.cc) restated here: which launcher runs, with which temporary
buffers, of which size. The wrappers allocate outputs without clearing them; this binding allocates every output
zero-filled (torch.zeros), so that memory a launcher never writes reads as 0 instead of garbage.

The launchers take device pointers, run on the null stream and copy synchronously; device buffers here are torch
tensors on the current device and every call is bracketed by torch.cuda.synchronize().

No prototype is written down. Each launcher is looked up at load time in `nm -D` / `nm -DC` of the built library by
its demangled name AND parameter list, the latter derived from the ctypes signature this binding passes
(computeAuxiliarBuffersSize has two overloads, so the name alone would not do).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import ref_build

# one letter per parameter: what the binding passes -> (ctypes type, spelling in a demangled parameter list)
_T = {"b": (C.c_bool, "bool"), "i": (C.c_int, "int"), "f": (C.c_float, "float"),
      "F": (C.c_void_p, "float const*"), "I": (C.c_void_p, "int const*"),
      "P": (C.c_void_p, "float*"), "Q": (C.c_void_p, "int*"), "B": (C.c_void_p, "bool*")}

#: key -> (launcher name, signature in the letters of _T, result). Argument order as the .cc wrappers call them.
LAUNCHERS = {
    "aabb": ("computeAABB", "biiFIPP", None),                                   # aabb_gpu.cc:79
    "num_cells": ("determineNumCells", "bifFF", C.c_int),                       # sort_gpu.cc:239
    "sort_aux": ("computeAuxiliarBuffersSize", "iiQQQ", None),                  # sort_gpu.cc:243
    "sort1": ("sortPointsStep1GPUKernel", "iiiFFFIQQQQQ", None),                # sort_gpu.cc:258-262
    "sort2": ("sortPointsStep2GPUKernel", "iiiiFIFIIQPQPQ", None),              # sort_gpu.cc:370-372
    "sort2_grad": ("sortPointsStep2GradGPUKernel", "iiFFIPP", None),            # sort_gpu.cc:424
    "feat_back": ("sortFeaturesBack", "iiFIP", None),                           # sort_gpu.cc:458
    "feat_back_grad": ("sortFeaturesBackGrad", "iiFIP", None),                  # sort_gpu.cc:491
    "inverse": ("computeInverseIndexs", "iIQ", None),                           # sort_gpu.cc:523
    "transform": ("transformIndexs", "iiIIQ", None),                            # sort_gpu.cc:531
    "count": ("countNeighborsCPU", "biifFIFIFFQ", C.c_uint),                    # find_neighbors.cc:153
    "neigh_aux": ("computeAuxiliarBuffersSize", "iQQ", None),                   # find_neighbors.cc:164
    "pack": ("packNeighborsCPU", "biiifFIFIFFQQQQ", None),                      # find_neighbors.cc:175-177
    "pdf": ("computeDPFsCPU", "bfiifFIFFIIP", None),                            # compute_pdf.cc:132
    "poisson": ("samplePointCloud", "bfiiiFFFIIPQQB", C.c_int),                 # poisson_sampling.cc:185
    "copy_points": ("copyPoints", "PQQiPQQ", None),                             # poisson_sampling.cc:203
    "sampled_feats": ("getFeaturesSampledPoints", "iiiIFP", None),              # poisson_sampling.cc:243
    "sampled_feats_grad": ("getFeaturesSampledPointsGradients", "iiiIFP", None),  # poisson_sampling.cc:286
    "conv": ("spatialConvCPU", "bbiiiibf" + "FIFFFII" + "FF" + "FFFFFF" + "P", None),           # spatial_conv.cc:308-310
    "conv_grad": ("spatialConvGradsCPU", "bbiiiiibf" + "FIFFFII" + "FF" + "FFFFFF" + "F" + "PPPPPPP", None),  # :505-508
}


def param_list(sig):
    """The demangled parameter list of a signature in the letters of _T, as `nm -DC` prints it."""
    return "(" + ", ".join(_T[c][1] for c in sig) + ")"


def dynamic_symbols(lib_path):
    """[(mangled, demangled)] of the functions the library defines, from `nm -D` and `nm -DC` (same order)."""
    def nm(*flags):
        out = subprocess.check_output(["nm", "-D", "--defined-only"] + list(flags) + [lib_path], text=True)
        return [ln.split(" ", 2) for ln in out.splitlines() if len(ln.split(" ", 2)) == 3]
    raw, dem = nm(), nm("-C")
    assert len(raw) == len(dem)
    syms = []
    for (a0, t0, m), (a1, t1, d) in zip(raw, dem):
        assert (a0, t0) == (a1, t1), (m, d)
        if t0 in "Tt":
            syms.append((m, d))
    return syms


def resolve(lib_path, table=None):
    """key -> list of mangled symbols whose demangled form is exactly `name(parameter list)` (exactly one is right)."""
    syms = dynamic_symbols(lib_path)
    out = {}
    for key, (name, sig, _) in (table or LAUNCHERS).items():
        want = name + param_list(sig)
        out[key] = [m for m, d in syms if d == want]
    return out


class Reference:
    """The reference's launchers behind the oracle's op surface. Needs a GPU and the built library."""

    def __init__(self, lib_path=None):
        import torch
        self.torch = torch
        path = lib_path or ref_build.LIB
        if not os.path.exists(path):
            raise FileNotFoundError(path + " is absent: run oracle/ref_build.py where the reference sources are")
        self.lib = C.CDLL(path)
        self.fn = {}
        for key, found in resolve(path).items():
            name, sig, res = LAUNCHERS[key]
            if len(found) != 1:
                raise RuntimeError("%s%s: %d symbols in %s" % (name, param_list(sig), len(found), path))
            f = getattr(self.lib, found[0])
            f.argtypes = [_T[c][0] for c in sig]
            f.restype = res
            self.fn[key] = f

    # -- helpers -----------------------------------------------------------
    def _sync(self):
        self.torch.cuda.synchronize()

    def _call(self, key, *args):
        """Device tensors go in as pointers; the launch is synchronised on both sides."""
        self._sync()
        r = self.fn[key](*[a.data_ptr() if isinstance(a, self.torch.Tensor) else a for a in args])
        self._sync()
        return r

    def _dev(self, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.size == 0:   # an empty tensor has no device pointer; the launchers never read past the counts they get
            return self.torch.zeros(1, dtype=self.torch.from_numpy(np.zeros(1, dtype)).dtype, device="cuda")
        return self.torch.from_numpy(a).cuda()

    def _f(self, a):
        return self._dev(a, np.float32)

    def _i(self, a):
        return self._dev(a, np.int32)

    def _zeros(self, n, dtype):
        return self.torch.zeros(max(int(n), 1), dtype=dtype, device="cuda")

    def _zf(self, n):
        return self._zeros(n, self.torch.float32)

    def _zi(self, n):
        return self._zeros(n, self.torch.int32)

    @staticmethod
    def _np(t, shape):
        n = int(np.prod(shape))
        return t.reshape(-1)[:n].cpu().numpy().reshape(shape).copy()

    def get_block_size(self):
        return ref_build.BLOCK_MLP_SIZE

    # -- op surface (MCConvModuleSrc), each following its .cc wrapper ---------
    def compute_aabb(self, inPts, inBatchIds, batchSize, scaleInv=True):
        # aabb_gpu.cc:51-79: two [B,3] outputs, one launcher (which fills them with +-FLT_MAX itself)
        pts, bids = self._f(inPts), self._i(np.asarray(inBatchIds).reshape(-1))
        mn, mx = self._zf(batchSize * 3), self._zf(batchSize * 3)
        self._call("aabb", bool(scaleInv), len(inPts), batchSize, pts, bids, mn, mx)
        return self._np(mn, (batchSize, 3)), self._np(mx, (batchSize, 3))

    def _num_cells(self, scaleInv, batchSize, cellSize, mn, mx):
        return int(self._call("num_cells", bool(scaleInv), batchSize, float(cellSize), mn, mx))

    def num_cells(self, aabbMin, aabbMax, batchSize, cellSize, scaleInv):
        return self._num_cells(scaleInv, batchSize, cellSize, self._f(aabbMin), self._f(aabbMax))

    def sort_points_step1(self, inPts, inBatchIds, aabbMin, aabbMax, batchSize, cellSize, scaleInv):
        # sort_gpu.cc:239-262: numCells from determineNumCells, three temporaries sized by the 5-argument
        # computeAuxiliarBuffersSize (counters per cell, per 512 cells, per 512*512 cells), then the launcher, which
        # clears the temporaries itself (sort_gpu.cu:454-462)
        n = len(inPts)
        pts, bids = self._f(inPts), self._i(np.asarray(inBatchIds).reshape(-1))
        mn, mx = self._f(aabbMin), self._f(aabbMax)
        nc = self._num_cells(scaleInv, batchSize, cellSize, mn, mx)
        s1, s2, s3 = C.c_int(0), C.c_int(0), C.c_int(0)
        self.fn["sort_aux"](batchSize, nc, C.addressof(s1), C.addressof(s2), C.addressof(s3))
        t1, t2, t3 = self._zi(s1.value), self._zi(s2.value), self._zi(s3.value)
        keys, idx = self._zi(n), self._zi(n)
        self._call("sort1", n, batchSize, nc, mn, mx, pts, bids, t1, t2, t3, keys, idx)
        return self._np(keys, (n,)), self._np(idx, (n,))

    def sort_points_step2(self, inPts, inBatchIds, inFeatures, keys, indexs, aabbMin, aabbMax, batchSize,
                          cellSize, scaleInv):
        # sort_gpu.cc:344-372: numCells again, outputs shaped like the inputs plus the [B,nc,nc,nc,2] cell table, one
        # int temporary per point (the sorted keys)
        feats = np.ascontiguousarray(inFeatures, np.float32)
        n, F = feats.shape
        pts, bids, fts = self._f(inPts), self._i(np.asarray(inBatchIds).reshape(-1)), self._f(feats)
        k, ix = self._i(keys), self._i(indexs)
        mn, mx = self._f(aabbMin), self._f(aabbMax)
        nc = self._num_cells(scaleInv, batchSize, cellSize, mn, mx)
        tmp = self._zi(n)
        oP, oB, oF, cells = self._zf(n * 3), self._zi(n), self._zf(n * F), self._zi(batchSize * nc ** 3 * 2)
        self._call("sort2", n, batchSize, F, nc, pts, bids, fts, k, ix, tmp, oP, oB, oF, cells)
        return (self._np(oP, (n, 3)), self._np(oB, (n, 1)), self._np(oF, (n, F)),
                self._np(cells, (batchSize, nc, nc, nc, 2)))

    def sort_points_step2_grad(self, indexs, ptsGrad, featGrad):
        # sort_gpu.cc:384-425
        pg, fg = np.ascontiguousarray(ptsGrad, np.float32), np.ascontiguousarray(featGrad, np.float32)
        n, F = fg.shape
        oP, oF = self._zf(n * 3), self._zf(n * F)
        self._call("sort2_grad", n, F, self._f(pg), self._f(fg), self._i(indexs), oP, oF)
        return self._np(oP, (n, 3)), self._np(oF, (n, F))

    def sort_features(self, inFeatures, indexs):
        # MCConvModuleSrc:35-36 calls the SortFeaturesBackGrad op; sort_gpu.cc:466-491
        f = np.ascontiguousarray(inFeatures, np.float32)
        n, F = f.shape
        out = self._zf(n * F)
        self._call("feat_back_grad", n, F, self._f(f), self._i(indexs), out)
        return self._np(out, (n, F))

    def sort_features_back(self, inFeatures, indexs):
        # sort_gpu.cc:433-458
        f = np.ascontiguousarray(inFeatures, np.float32)
        n, F = f.shape
        out = self._zf(n * F)
        self._call("feat_back", n, F, self._f(f), self._i(indexs), out)
        return self._np(out, (n, F))

    def sort_features_back_grad(self, indexs, featGrad):
        return self.sort_features(featGrad, indexs)

    def transform_indexs(self, inIndexs, inNewPositions):
        # sort_gpu.cc:500-531: invert the permutation into a temporary, then look the indices up in it
        a, b = np.asarray(inIndexs).reshape(-1), np.asarray(inNewPositions).reshape(-1)
        tmp, out = self._zi(len(b)), self._zi(len(a))
        self._call("inverse", len(b), self._i(b), tmp)
        self._call("transform", len(a), len(b), self._i(a), tmp, out)
        return self._np(out, (len(a),))

    def find_neighbors(self, inPts, inBatchIds, inPts2, cellIndexs, aabbMin, aabbMax, radius, batchSize, scaleInv):
        # find_neighbors.cc:93-177: numCells is the cell table's second dimension; count (per-centre counts land in
        # startIndexs, the total comes back), size the [total,2] output, two offset temporaries from the 3-argument
        # computeAuxiliarBuffersSize (one per 256 centres, one per 256*256), then pack
        m = len(inPts)
        cells_np = np.ascontiguousarray(cellIndexs, np.int32)
        nc = cells_np.shape[1]
        c, cb, p2, cells = self._f(inPts), self._i(np.asarray(inBatchIds).reshape(-1)), self._f(inPts2), self._i(cells_np)
        mn, mx = self._f(aabbMin), self._f(aabbMax)
        start = self._zi(m)
        tot = int(self._call("count", bool(scaleInv), m, nc, float(radius), c, cb, p2, cells, mn, mx, start))
        s1, s2 = C.c_int(0), C.c_int(0)
        self.fn["neigh_aux"](m, C.addressof(s1), C.addressof(s2))
        t1, t2 = self._zi(s1.value), self._zi(s2.value)
        packed = self._zi(tot * 2)
        self._call("pack", bool(scaleInv), m, tot, nc, float(radius), c, cb, p2, cells, mn, mx, t1, t2, start, packed)
        return self._np(start, (m, 1)), self._np(packed, (tot, 2))

    def compute_pdf(self, inPts, inBatchIds, aabbMin, aabbMax, startIndexs, neighbors, window, radius, batchSize,
                    scaleInv):
        # compute_pdf.cc:73-133: numSamples = rows of startIndexs, numNeighs = rows of the packed list
        st, pk = np.asarray(startIndexs).reshape(-1), np.ascontiguousarray(neighbors, np.int32)
        e = len(pk)
        out = self._zf(e)
        if e:   # a launch of zero blocks is an error on either runtime
            self._call("pdf", bool(scaleInv), float(window), len(st), e, float(radius), self._f(inPts),
                       self._i(np.asarray(inBatchIds).reshape(-1)), self._f(aabbMin), self._f(aabbMax), self._i(st),
                       self._i(pk), out)
        return self._np(out, (e, 1))

    def poisson_sampling(self, inPts, inBatchIds, cellIndexs, aabbMin, aabbMax, radius, batchSize, scaleInv):
        # poisson_sampling.cc:124-203: four per-point temporaries (points, batch ids, indices, the "selected" flags;
        # the launcher clears the flags), the launcher returns the count, copyPoints moves that many rows to the outputs
        n = len(inPts)
        cells_np = np.ascontiguousarray(cellIndexs, np.int32)
        nc = cells_np.shape[1]
        tP, tB, tI = self._zf(n * 3), self._zi(n), self._zi(n)
        used = self._zeros(n, self.torch.bool)
        s = int(self._call("poisson", bool(scaleInv), float(radius), n, batchSize, nc, self._f(aabbMin),
                           self._f(aabbMax), self._f(inPts), self._i(np.asarray(inBatchIds).reshape(-1)),
                           self._i(cells_np), tP, tB, tI, used))
        oP, oB, oI = self._zf(s * 3), self._zi(s), self._zi(s)
        self._call("copy_points", tP, tB, tI, s, oP, oB, oI)
        return self._np(oP, (s, 3)), self._np(oB, (s, 1)), self._np(oI, (s,))

    def get_sampled_features(self, inSampledIndexs, pInFeatures):
        # poisson_sampling.cc:218-243
        f = np.ascontiguousarray(pInFeatures, np.float32)
        idx = np.asarray(inSampledIndexs).reshape(-1)
        n, F = f.shape
        out = self._zf(len(idx) * F)
        self._call("sampled_feats", n, F, len(idx), self._i(idx), self._f(f), out)
        return self._np(out, (len(idx), F))

    def get_sampled_features_grad(self, inSampledIndexs, pInFeatures, grads):
        # poisson_sampling.cc:252-286 (the launcher clears the output)
        n, F = np.asarray(pInFeatures).shape
        idx = np.asarray(inSampledIndexs).reshape(-1)
        out = self._zf(n * F)
        self._call("sampled_feats_grad", n, F, len(idx), self._i(idx), self._f(grads), out)
        return self._np(out, (n, F))

    def _conv_args(self, inPts, inFeatures, inBatchIds, inPDFs, inSamplePts, neighStartIndexs, packedNeighs,
                   aabbMin, aabbMax, weights1, weights2, weightsOut, biases1, biases2, biasesOut):
        # spatial_conv.cc:182-300: every tensor goes in flat, in its declared memory order
        flat = lambda a: np.asarray(a).reshape(-1)
        return [self._f(inPts), self._i(flat(inBatchIds)), self._f(inFeatures), self._f(flat(inPDFs)),
                self._f(inSamplePts), self._i(flat(neighStartIndexs)), self._i(packedNeighs),
                self._f(aabbMin), self._f(aabbMax), self._f(flat(weights1)), self._f(flat(biases1)),
                self._f(flat(weights2)), self._f(flat(biases2)), self._f(flat(weightsOut)), self._f(flat(biasesOut))]

    def spatial_conv(self, inPts, inFeatures, inBatchIds, inPDFs, inSamplePts, neighStartIndexs, packedNeighs,
                     aabbMin, aabbMax, weights1, weights2, weightsOut, biases1, biases2, biasesOut,
                     numOutFeatures, combin, batchSize, radius, scaleInv, avg):
        # spatial_conv.cc:180-310: numNeighs = rows of the pdfs, numSamples = rows of the sample points
        a = self._conv_args(inPts, inFeatures, inBatchIds, inPDFs, inSamplePts, neighStartIndexs, packedNeighs,
                            aabbMin, aabbMax, weights1, weights2, weightsOut, biases1, biases2, biasesOut)
        fin = np.asarray(inFeatures).shape[1]
        m, e = len(inSamplePts), len(packedNeighs)
        outF = numOutFeatures if combin else fin
        out = self._zf(m * outF)
        if e:
            self._call("conv", bool(avg), bool(scaleInv), e, fin, numOutFeatures, m, bool(combin), float(radius),
                       *a, out)
        return self._np(out, (m, outF))

    def spatial_conv_grad(self, inPts, inFeatures, inBatchIds, inPDFs, inSamplePts, neighStartIndexs,
                          packedNeighs, aabbMin, aabbMax, weights1, weights2, weightsOut, biases1, biases2,
                          biasesOut, outGrad, numOutFeatures, combin, batchSize, radius, scaleInv, avg):
        # spatial_conv.cc:344-508: seven outputs shaped like the features and the six parameter tensors. The launcher
        # clears what it is going to accumulate into (spatial_conv.cu:919-925, 940-946) -- of dw3 / db3 only the first
        # fin*fout (combin) or fin rows, so the rows of padded output neurons are whatever the buffer held: zeros here.
        a = self._conv_args(inPts, inFeatures, inBatchIds, inPDFs, inSamplePts, neighStartIndexs, packedNeighs,
                            aabbMin, aabbMax, weights1, weights2, weightsOut, biases1, biases2, biasesOut)
        n, fin = np.asarray(inFeatures).shape
        m, e = len(inSamplePts), len(packedNeighs)
        nn = np.asarray(biases1).size
        fg = self._zf(n * fin)
        dw1, db1, dw2, db2, dw3, db3 = (self._zf(3 * nn), self._zf(nn), self._zf(8 * nn), self._zf(nn),
                                        self._zf(8 * nn), self._zf(nn))
        if e:
            self._call("conv_grad", bool(avg), bool(scaleInv), e, fin, numOutFeatures, m, n, bool(combin),
                       float(radius), *a, self._f(outGrad), fg, dw1, dw2, dw3, db1, db2, db3)
        g = self._np
        return (g(fg, (n, fin)), g(dw1, (3, nn)), g(db1, (nn,)), g(dw2, (8, nn)), g(db2, (nn,)), g(dw3, (8, nn)),
                g(db3, (nn,)))
