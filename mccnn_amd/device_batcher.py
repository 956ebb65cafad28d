"""Training batches built on the GPU: the device counterpart of mccnn_amd.batcher.RaggedBatcher.

The models are uploaded once into a store on the device (points concatenated, optionally normals, features, labels, and a
host offset table). After that a batch costs the host one small record per slot -- the PLAN -- and the GPU does the
per-point work: csrc/batch_sample.hip selects the points of every slot by its sampling protocol, rotates them, writes the
batch ids and the store row behind every output row; feature and label rows follow through that index with
mccnn_permute_gather / a torch gather on the same stream. The slot, iterator, maxPtsxBatch and repeatModelInBatch rules are
RaggedBatcher's, and the plan is drawn from the batcher's RandomState with the host batcher's calls in its order (protocol
choice, `random_view` for lambert and occlusion, the rotation of `_augment_data_rot_`). The per-slot uint32 seed of the
per-point draws comes from a second RandomState, so that the main generator is consumed exactly as far as the host batcher
consumes it outside its sampling functions.

WHERE THIS DEPARTS FROM THE REFERENCE LOADER (RaggedBatcher stays the bit-identical one):
  1. Counter-based draws. The per-point draws are a hash of (seed, pass, point index) (csrc/batch_sample.h), not numbers
     taken from the RandomState one by one: a run is reproducible from its seed and follows the reference's protocols and
     probabilities, but it is NOT the reference's random stream.
  2. The uniform protocol is a STRATIFIED sample, not a simple random one: row t of K reads one point of stratum
     [floor(t n / K), floor((t + 1) n / K)), which gives K distinct indices in ascending order with inclusion probability
     1 / len_t (len_t = floor(n / K) or ceil(n / K)) -- `RandomState.choice` without replacement returns a uniformly random
     subset in random order. With n < K (the host draws with replacement) every row draws independently.
  3. The pass bound and its status codes. Split, gradient and lambert repeat passes over a model until numPoints rows are
     collected, at most mccnn_batch_max_passes() (64) of them. A slot whose first pass accepts nothing (lambert with no
     normal towards the view, occlusion with no facing point) ends with status NO_POINT -- also where the host loop would
     have gone on drawing because some probability is positive -- and one that is short of its rows after the last pass with
     status PASS_BOUND; both fill their missing rows with the model's row 0. `check=True` raises for them.
All protocols are evaluated in f32 (the host functions work in f64); tests/device_batcher_ref.py restates them in NumPy
float32 and the kernel agrees with that bit for bit.
"""
import contextlib
import time

import numpy as np

from . import sampling

# one record per slot: mccnn_batch_slot of include/mccnn.h, field by field
SLOT_DTYPE = np.dtype([("offset", "<i4"), ("length", "<i4"), ("protocol", "<i4"), ("rows", "<i4"), ("out_base", "<i4"),
                       ("batch_id", "<i4"), ("n_sel", "<i4"), ("exact", "<i4"), ("seed", "<u4"), ("view", "<f4", (3,)),
                       ("rot", "<f4", (9,)), ("bmin", "<f4", (3,)), ("bmax", "<f4", (3,))], align=True)
assert SLOT_DTYPE.itemsize == 108

STATUS_OK, STATUS_NO_POINT, STATUS_PASS_BOUND = 0, 1, 2


def new_slots(count):
    """`count` zeroed slot records with the identity rotation."""
    s = np.zeros(count, SLOT_DTYPE)
    s["rot"] = np.eye(3, dtype=np.float32).reshape(9)
    return s


class DeviceStore:
    """The models of a data set, concatenated on the device. pts f32 [P,3]; normals f32 [P,3], features f32 [P,F] and
    labels [P,L] when every model carries them; host tables: offsets [M+1], box minimum / maximum [M,3] in f32."""

    def __init__(self, models, device="cuda"):
        import torch
        models = list(models)
        has = lambda k: len(models) > 0 and all(m.get(k) is not None for m in models)
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(m[k]).reshape(len(m["pts"]), -1) for m in models], axis=0), dtype=dt)
        lengths = np.array([len(m["pts"]) for m in models], np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        if self.offsets[-1] >= 2 ** 31:
            raise RuntimeError("the store is indexed with int32")
        self.lengths = lengths
        self.device = torch.device(device)
        pts = cat("pts", np.float32) if len(models) else np.zeros((0, 3), np.float32)
        self.bmin = np.zeros((len(models), 3), np.float32)
        self.bmax = np.zeros((len(models), 3), np.float32)
        for k in range(len(models)):
            if lengths[k] > 0:
                seg = pts[self.offsets[k]:self.offsets[k + 1]]
                self.bmin[k], self.bmax[k] = seg.min(axis=0), seg.max(axis=0)
        up = lambda a: torch.from_numpy(a).to(self.device)
        self.pts = up(pts)
        self.normals = up(cat("normals", np.float32)) if has("normals") else None
        self.features = up(cat("features", np.float32)) if has("features") else None
        self.labels = None
        if has("labels"):
            lab = np.concatenate([np.asarray(m["labels"]).reshape(len(m["pts"]), -1) for m in models], axis=0)
            self.labels = up(np.ascontiguousarray(lab, dtype=np.float32 if lab.dtype.kind == "f" else lab.dtype))

    def fill_model(self, slot, model):
        """offset, length, n_sel and box of model `model` into the record `slot` (one element of a SLOT_DTYPE array)."""
        slot["offset"], slot["length"] = self.offsets[model], self.lengths[model]
        slot["n_sel"] = self.lengths[model]
        slot["bmin"], slot["bmax"] = self.bmin[model], self.bmax[model]


def sample_plan(store, slots, out_rows, stream=None):
    """One plan through the kernel: -> (pts f32 [out_rows,3], batch ids i32 [out_rows,1], src i32 [out_rows], counts i32
    [S], status i32 [S]) on the store's device, built on `stream` (torch's current stream when None). `src` holds the store
    row behind every output row. Launches: one per 32 slots."""
    import torch
    from . import _lib
    if store.device.type != "cuda":
        raise _lib.MCCNNError("a batch is built by the HIP kernel: the store has to live on the GPU (there is no host fall-back)")
    lib = _lib.load()
    slots = np.ascontiguousarray(slots, dtype=SLOT_DTYPE)
    S = len(slots)
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        dev = store.device
        pts = torch.empty((out_rows, 3), dtype=torch.float32, device=dev)
        bids = torch.empty((out_rows, 1), dtype=torch.int32, device=dev)
        src = torch.empty((out_rows,), dtype=torch.int32, device=dev)
        cs = torch.empty((2, max(S, 1)), dtype=torch.int32, device=dev)
        _lib.check(lib.mccnn_batch_sample(_lib.ptr(store.pts), _lib.ptr(store.normals), store.pts.shape[0], slots.ctypes.data, S,
                                          out_rows, _lib.ptr(pts), _lib.ptr(bids), _lib.ptr(src), _lib.ptr(cs[0]), _lib.ptr(cs[1]),
                                          _lib.stream_handle()), "mccnn_batch_sample")
    return pts, bids, src, cs[0, :S], cs[1, :S]


class DeviceBatcher:
    """RaggedBatcher's constructor arguments plus `device`; the same start_iteration / has_more_batches / get_num_models.
    `get_next_batch` returns RaggedBatcher's 7-tuple with DEVICE tensors: points f32 [N,3], batch ids i32 [N,1], features
    f32 [N,F] (ones [N,1] when the models carry none), labels or None, categories (int64 tensor) or None, and the model ids
    as a host list."""

    def __init__(self, models, numPoints, ptDropOut, batchSize, allowedSamplings, categories=None, pointCategories=False,
                 maxPtsxBatch=0, augment=False, augmentMainAxis=1, augmentSmallRotations=False, uniformSelectFirst=False,
                 augmentedFeatures=(), augmentedLabels=(), seed=None, device="cuda"):
        if not (0 <= augmentMainAxis < 3):
            raise RuntimeError('Invalid augmentMainAxis')
        if not all(0 <= s < 5 for s in allowedSamplings):
            raise RuntimeError('Invalid sampling protocol')
        models = list(models)
        self.store_ = DeviceStore(models, device)
        self.numModels_ = len(models)
        self.pointNormals_ = self.store_.normals is not None
        self.pointFeatures_ = self.store_.features is not None
        self.pointLabels_ = self.store_.labels is not None
        if (3 in list(allowedSamplings) or 4 in list(allowedSamplings)) and not self.pointNormals_:
            raise RuntimeError('The dataset should contain normals in order to use the sampling protocols '
                               'lambert and occlusion')
        for lst in (augmentedFeatures, augmentedLabels):
            if any(lst[i + 1] - lst[i] < 3 for i in range(max(len(lst) - 1, 0))):
                raise RuntimeError('The groups of 3 features/labels to augment should not overlap ')
        if any(n == 0 for n in self.store_.lengths):
            raise RuntimeError('A model without points cannot be sampled')
        self.numPoints_ = numPoints
        self.ptDropOut_ = ptDropOut
        self.useCategories_ = categories is not None
        self.pointCategories_ = pointCategories
        self.categories_ = list(categories) if categories is not None else []
        self.batchSize_ = batchSize
        self.allowedSamplings_ = allowedSamplings
        self.maxPtsxBatch_ = maxPtsxBatch
        self.augment_ = augment
        self.augmentMainAxis_ = augmentMainAxis
        self.augmentSmallRotations_ = augmentSmallRotations
        self.augmentedFeatures_ = list(augmentedFeatures)
        self.augmentedLabels_ = list(augmentedLabels)
        self.uniformSelectFirst_ = uniformSelectFirst
        self.numPts_ = [int(n) for n in self.store_.lengths]
        self.randomSelection_ = []
        self.iterator_ = 0
        seed = seed if seed is not None else int(time.time())
        self.randomState_ = np.random.RandomState(seed)
        self.seedState_ = np.random.RandomState((int(seed) + 0x9E3779B9) % (2 ** 32))   # the per-slot seeds: see the module docstring
        self.lastLaunches_ = 0   # launches of the last get_next_batch: the kernel's plus the gathers

    # ------------------------------------------------------------------ iteration protocol: RaggedBatcher's
    def get_num_models(self):
        return self.numModels_

    def start_iteration(self):
        self.randomSelection_ = self.randomState_.permutation(self.numModels_)
        self.iterator_ = 0

    def has_more_batches(self):
        return self.iterator_ < len(self.randomSelection_)

    def _rotation_(self):
        """The matrix `_augment_data_rot_` draws (RaggedBatcher, DataSet.py:252-311): the same calls in the same order."""
        rs = self.randomState_
        rotationAngle = rs.uniform() * 2.0 * np.pi
        c, s = np.cos(rotationAngle), np.sin(rotationAngle)
        if self.augmentMainAxis_ == 0:
            rot = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
        elif self.augmentMainAxis_ == 1:
            rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
        else:
            rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        if self.augmentSmallRotations_:
            a = np.clip(0.06 * rs.randn(3), -0.18, 0.18)
            Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a[0]), -np.sin(a[0])], [0.0, np.sin(a[0]), np.cos(a[0])]])
            Ry = np.array([[np.cos(a[1]), 0.0, np.sin(a[1])], [0.0, 1.0, 0.0], [-np.sin(a[1]), 0.0, np.cos(a[1])]])
            Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0.0], [np.sin(a[2]), np.cos(a[2]), 0.0], [0.0, 0.0, 1.0]])
            rot = np.dot(np.dot(Rz, np.dot(Ry, Rx)), rot)
        return rot

    # ------------------------------------------------------------------ the plan: everything the host contributes to a batch
    def plan_batch(self, repeatModelInBatch=False):
        """Advances the iterator and the generators by one batch and returns its plan: dict with `slots` (SLOT_DTYPE array,
        one record per model of the batch), `ids`, `numModelInBatch`, `categories` (per model, or None), `out_rows` (rows of
        the kernel's output buffers) and `exact` (numPoints > 0: every slot produces exactly numPoints rows and nothing is
        read back)."""
        rs = self.randomState_
        st = self.store_
        slots = new_slots(self.batchSize_)
        ids = []
        k = 0
        numPtsInBatch = 0
        out_rows = 0
        for i in range(self.batchSize_):
            if self.iterator_ >= len(self.randomSelection_):
                continue
            idx = int(self.randomSelection_[self.iterator_])
            n = self.numPts_[idx]
            if not (self.maxPtsxBatch_ == 0 or (numPtsInBatch + n) <= self.maxPtsxBatch_):
                continue
            s = slots[k]
            st.fill_model(s, idx)
            proto = int(rs.choice(self.allowedSamplings_))
            s["protocol"] = proto
            if proto >= 3:
                s["view"] = sampling.random_view(rs)
            if self.augment_:
                s["rot"] = self._rotation_().reshape(9)
            s["seed"] = self.seedState_.randint(0, 2 ** 32, dtype=np.uint32)
            s["batch_id"] = i
            s["out_base"] = out_rows
            if self.numPoints_ > 0:
                s["exact"] = 1
                s["rows"] = self.numPoints_
                if proto == 0 and self.uniformSelectFirst_ and n >= self.numPoints_:
                    s["n_sel"] = min(n, int(float(self.numPoints_) * (2.0 - self.ptDropOut_)))
            else:
                s["rows"] = int(float(n) * self.ptDropOut_) if proto == 0 else n
            out_rows += int(s["rows"])
            ids.append(idx)
            numPtsInBatch += n
            k += 1
            if not repeatModelInBatch:
                self.iterator_ += 1
        if repeatModelInBatch:
            self.iterator_ += 1
        return {"slots": slots[:k].copy(), "ids": ids, "numModelInBatch": k, "out_rows": out_rows, "exact": self.numPoints_ > 0,
                "categories": [self.categories_[i] for i in ids] if self.useCategories_ else None}

    # ------------------------------------------------------------------ the batch
    def build_batch(self, plan, stream=None, check=True):
        """One plan of `plan_batch` through the GPU -> get_next_batch's result."""
        import torch
        from . import _lib
        st = self.store_
        slots, S = plan["slots"], plan["numModelInBatch"]
        cur = torch.cuda.current_stream(st.device)
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            pts, bids, src, counts, status = sample_plan(st, slots, plan["out_rows"])
            launches = (S + 31) // 32
            counts_h = None
            if not plan["exact"]:
                # the one read-back of this mode: the B counts (and, with them, the status words) cut the result
                cs = torch.stack([counts, status]).cpu().numpy()
                counts_h, status_h = cs[0], cs[1]
                keep = np.concatenate([np.arange(b, b + c) for b, c in zip(slots["out_base"], counts_h)] + [np.zeros(0, np.int64)])
                keep = torch.from_numpy(keep.astype(np.int64)).to(st.device)
                pts, bids, src = pts.index_select(0, keep), bids.index_select(0, keep), src.index_select(0, keep)
            elif check:
                status_h = status.cpu().numpy()
            N = pts.shape[0]
            rows_of = counts_h if counts_h is not None else slots["rows"]
            rank = None   # slot rank of every row, for what differs per slot: the rotation, the category

            def slot_rank():
                return torch.repeat_interleave(torch.arange(S, device=st.device), torch.from_numpy(np.asarray(rows_of, np.int64)).to(st.device),
                                               output_size=N)

            def gather(table, blocks):
                nonlocal rank, launches
                if table.dtype == torch.float32 and N > 0:
                    out = torch.empty((N, table.shape[1]), dtype=torch.float32, device=st.device)
                    _lib.check(_lib.load().mccnn_permute_gather(_lib.ptr(table), _lib.ptr(src), N, table.shape[1], _lib.ptr(out),
                                                                _lib.stream_handle()), "mccnn_permute_gather")
                else:
                    out = table.index_select(0, src.long())
                launches += 1
                if self.augment_ and blocks and N > 0 and out.dtype.is_floating_point:
                    if rank is None:
                        rank = slot_rank()
                    rot = torch.from_numpy(np.ascontiguousarray(slots["rot"].reshape(S, 3, 3))).to(st.device)[rank]
                    for blk in blocks:
                        out[:, blk:blk + 3] = (out[:, blk:blk + 3].unsqueeze(2) * rot).sum(1)
                return out

            feats = gather(st.features, self.augmentedFeatures_) if self.pointFeatures_ else torch.ones((N, 1), dtype=torch.float32, device=st.device)
            labels = gather(st.labels, self.augmentedLabels_) if self.pointLabels_ else None
            cats = None
            if self.useCategories_:
                cats = torch.tensor([self.categories_[i] for i in plan["ids"]], device=st.device)
                if self.pointCategories_:
                    rank = slot_rank() if rank is None else rank
                    cats = cats[rank].reshape(-1, 1)
            if stream is not None and stream != cur:
                for t in (pts, bids, feats, labels, cats, status):
                    if t is not None:
                        t.record_stream(cur)
        self.lastLaunches_ = launches
        if check:
            if np.any(status_h == STATUS_NO_POINT):
                raise RuntimeError("no point can be selected")
            if np.any(status_h == STATUS_PASS_BOUND):
                raise RuntimeError("a slot is short of its points after %d passes over its model" % _lib.load().mccnn_batch_max_passes())
        out = (S, pts, bids, feats, labels, cats, plan["ids"])
        return out if check else out + (status,)

    def get_next_batch(self, repeatModelInBatch=False, stream=None, check=True):
        """-> (numModelInBatch, pts [N,3], batch ids [N,1], features [N,F], labels or None, categories or None, ids), built
        on `stream` (torch's current stream when None; the caller orders its consumers behind that stream). check=True reads
        the status words back once the batch is complete and raises RuntimeError("no point can be selected") or the
        pass-bound error; check=False appends the status tensor [numModelInBatch] to the tuple instead and, with
        numPoints > 0, does not wait for the device at all. With numPoints == 0 the per-slot counts are read back once."""
        return self.build_batch(self.plan_batch(repeatModelInBatch), stream=stream, check=check)
