"""Native step executor (csrc/exec.hip, include/mccnn.h "NATIVE STEP EXECUTOR"): what
ConvolutionBuilder.create_convolution does around the kernels -- grid, neighbour list, PDFs, feature sort, kernel
choice, row plans -- behind one library call per convolution GEOMETRY and one per layer and direction.

A step of a network is bound by the host issuing its launches: ~12 us of Python per launch against 3 us for
the launch itself. This module is the thin remainder: it owns the device buffers the library asks for (the library
never allocates), the pinned word the edge total arrives in, and the autograd node of a layer.
"""
import os
import ctypes as C
import threading
import weakref

import torch

from . import _env, _lib
from ._lib import check, ptr, stream_handle
from .MCConvModule import _edge_guess, _remember_edges, _ws, _bf16_rows_aligned
from . import dense_glue as M   # (behind MCConvModule, whose import brings dense_glue in)


def _load_ext():
    """mccnn_amd/lib/_mccnn_torch.so (csrc/torch_ext.cpp): the same calls as below from C++, with the autograd node on the
    C++ side -- a convolution then costs the host one Python -> C++ call forward and none backward. MCCNN_TORCH_EXT=0 (or a
    tree without the built module) keeps the ctypes form."""
    import importlib.util
    if not _env.flag("TORCH_EXT"):
        return None
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "_mccnn_torch.so")
    if not os.path.exists(path):
        return None
    _lib.load()  # libmccnn_hip.so first: the module links against it (a missing HIP library raises: no fallback for that)
    try:
        spec = importlib.util.spec_from_file_location("_mccnn_torch", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    except (ImportError, OSError) as err:  # built against another torch: the ctypes binding of the SAME library takes over
        import sys
        print("mccnn_amd.native: lib/_mccnn_torch.so does not load (%s); using the ctypes binding of libmccnn_hip.so" % err,
              file=sys.stderr)
        return None
    return mod


_EXT = _load_ext()
if _EXT is not None:
    # The extension's helper threads hold tensors that have Python objects; dropping the last reference to one takes the
    # GIL, and a non-main thread that asks for it while the interpreter finalises is ended by Python with a forced unwind
    # (std::terminate: "terminate called without an active exception" at the end of a script that stops with prefetched
    # work in flight). Before finalisation starts the queued jobs are run to the end and the threads joined.
    import atexit
    atexit.register(_EXT.shutdown_helpers)

E_CAPACITY = -6
NEED_PLAN_FWD, NEED_PLAN_TR, NEED_TLIST, NEED_RECORDS = 1, 2, 4, 8      # mccnn.h: MCCNN_PIECE_*
CONV_KEEP_STATE, CONV_DETERMINISTIC, CONV_READS_RECORDS = 1, 2, 4        # mccnn.h: MCCNN_CONV_*, the flags of mccnn_conv_*

_TLS = threading.local()
_EDGE_GUESS = {}   # (device, n, m, radius, B, scaleInv[, maxNeighbors]) -> capacity to try first
_EDGE_RATIO = {}   # (device, radius, scaleInv[, maxNeighbors]) -> edges per centre of the last search with this radius


def _slot():
    """A pinned int32 the count pass stores the edge total into (device-accessible host memory: no copy is enqueued);
    pooled per host thread."""
    _poll_parked()
    pool = getattr(_TLS, "slots", None)
    if pool is None:
        pool = _TLS.slots = []
    if pool:
        return pool.pop()
    return torch.empty(1, dtype=torch.int32).pin_memory()


def _release_slot(t):
    pool = getattr(_TLS, "slots", None)
    if pool is not None and len(pool) < 64:
        pool.append(t)


_PARKED = []   # (slot, event): words of geometries dropped before their total arrived -- the count pass may still write them
_PARKED_LOCK = threading.Lock()   # Geometry.__del__ parks from any thread, and from GC runs inside _poll_parked's own loop


def _park_slot(t):
    """Keeps a pinned word alive (neither pooled nor returned to the host allocator) until everything the current stream
    holds -- the build that writes it among it -- has retired."""
    try:
        ev = torch.cuda.Event()
        ev.record()
    except Exception:   # interpreter shutdown, no device: the word simply stays referenced
        ev = None
    _PARKED.append((t, ev))   # (list.append is atomic; _poll_parked never overwrites the list, see there)


def _poll_parked():
    if not _PARKED:
        return
    # Take the entries present NOW out of the list in one atomic step and work on the private copy: an entry parked while
    # this loop runs (another thread, or a GC run triggered by the allocations below calling Geometry.__del__) stays in
    # _PARKED and is never dropped -- `_PARKED[:] = keep` used to discard it and hand a word the count pass could still
    # write back to the host allocator. Non-blocking: a second caller simply skips its poll.
    if not _PARKED_LOCK.acquire(False):
        return
    try:
        k = len(_PARKED)
        items = _PARKED[:k]
        del _PARKED[:k]
        keep = []
        for t, ev in items:
            try:
                done = int(t[0]) >= 0 or ev is None or ev.query()
            except Exception:
                done = False
            if done:
                _release_slot(t)
            else:
                keep.append((t, ev))
        _PARKED.extend(keep)
    finally:
        _PARKED_LOCK.release()


_KDE_RECORDS = _env.debug("kde_records", True)   # (0: no geometry is asked for per-edge records -- A/B)
_ECAP_SCALE = _env.debug("ecap_scale", 1.0)   # (debugging: generous / starved capacity guesses)


def _capacity_guess(gkey, m):
    g = _edge_guess(_EDGE_GUESS, _EDGE_RATIO, gkey, m, 48 * m + 1024)   # (first search of a radius: a plain guess)
    return int(g * _ECAP_SCALE) + 1024 if _ECAP_SCALE != 1.0 else g


def _remember(gkey, m, e):
    _remember_edges(_EDGE_GUESS, _EDGE_RATIO, gkey, m, e)


class _NeighborCap(C.Structure):
    """mccnn_neighbor_cap (include/mccnn.h)"""
    _fields_ = [("max_neighbors", C.c_int), ("sampled", C.c_int), ("seed", C.c_uint)]


class _NeighborBudget(C.Structure):
    """mccnn_neighbor_budget (include/mccnn.h)"""
    _fields_ = [("max_edges", C.c_int)]


class _PointPdf(C.Structure):
    """mccnn_point_pdf (include/mccnn.h)"""
    _fields_ = [("density", C.c_void_p), ("counts", C.c_void_p), ("ready", C.c_int)]


class Geometry:
    """One convolution geometry: the grid of the input level at the convolution radius, the neighbour list of the
    output level's points in it and its PDFs, in ONE device buffer (mccnn_geometry_t). Tensor views of its arrays are
    made on demand (grid(), neighbors(), pdfs()) -- the layers themselves only hand the handle to the library."""

    def __init__(self):
        self.core = None        # the C++ object of the torch extension (owns handle / buffers), when that is in use
        self.handle = None
        self.buf = None
        self.slot = None
        self.keep = None        # the input tensors the library borrowed pointers of
        self.attached = []      # plan / list buffers handed to the library
        self.grid_owner = None
        self.n = self.m = self.nc = self.B = self.e_cap = 0
        self.e = -1
        self.gkey = None
        self.args = None
        self.cap = (0, None)    # (maxNeighbors, sampleSeed) of the search
        self.budget = 0         # maxEdges of the search (0: none): the search picks the cap itself, chosen_cap()
        self.point = False      # the PDFs are expanded from the per-point density of (grid, window): pdfMode='point'
        self.window = None
        self.recordsAvg = None  # the `avg` of the per-edge records the build's KDE was asked to leave (None: not asked)
        # a grid owner: window -> (density [n,1] f32, counts [n,1] i32, handle of the extension or None) of its sorted points --
        # ONE pair per window, shared by every geometry over this grid (alive as long as the owner is)
        self.pointPairs = {}
        self.uses = 0           # layers convolved over this geometry so far (the builder counts)

    def __del__(self):
        h, self.handle = self.handle, None
        if h is not None:
            try:
                _lib.load().mccnn_geometry_destroy(h)
            except Exception:
                pass
        if self.slot is not None:
            if self.e >= 0:
                _release_slot(self.slot)
            else:   # the total never arrived here: the count pass may still write the word (see _park_slot)
                try:
                    _park_slot(self.slot)
                except Exception:
                    pass

    # ------------------------------------------------------------------ sizes
    def edges(self):
        """E (waits for the count pass of the build)."""
        if self.e < 0:
            e = self.core.edges(-1) if self.core is not None else _lib.load().mccnn_geometry_edges(self.handle, -1)
            if e < 0:
                raise _lib.MCCNNError("geometry: edge total not available")
            self.e = e
            _remember(self.gkey, self.m, e)
            if e > self.e_cap:
                self._rebuild(e + e // 16 + 64)
        return self.e

    def _rebuild(self, capacity):
        """The neighbour list was longer than the guess: exact repeat (first batch of a shape)."""
        inPts, inBids, centres, cbids, mn, mx, B, nc, radius, scaleInv, window, usePDF = self.args
        if self.cap[0] > 0:   # (a capped list never holds more)
            capacity = min(capacity, self.m * self.cap[0])
        if self.budget > 0:   # (nor does a budgeted one hold more than max(B, m) rows)
            capacity = min(capacity, max(self.budget, self.m))
        # (a per-point density does not depend on the list: the one that exists is expanded again, not computed again)
        _build_into(self, inPts, inBids, centres, cbids, mn, mx, B, nc, radius, scaleInv, window, usePDF, capacity,
                    self.grid_owner, maxNeighbors=self.cap[0], sampleSeed=self.cap[1], pointPDF=self.point, maxEdges=self.budget,
                    recordsAvg=self.recordsAvg)
        e = self.core.edges(-1) if self.core is not None else _lib.load().mccnn_geometry_edges(self.handle, -1)
        if e < 0 or e > self.e_cap:
            raise _lib.MCCNNError("geometry: rebuilt list still does not fit (%d > %d)" % (e, self.e_cap))
        self.e = e

    def prebuild(self, what, avg, side, like):
        """Row plans / transposed list ahead of the layers that need them, on a side stream (torch extension only);
        what: NEED_* mask. Waits for the edge total."""
        if self.core is not None:
            self.edges()
            self.core.prebuild(int(what), bool(avg), int(side), like)

    @property
    def have(self):
        """Mask of the pieces attached so far (NEED_*)."""
        return int(self.core.have) if self.core is not None else 0

    def prebuild_async(self, what, avg):
        """Pieces of a geometry whose build has just been queued on a side stream: buffers allocated now (bounds over
        the capacity), attached and issued by the extension's helper thread once the edge total has arrived -- the
        calling thread does not wait."""
        if self.core is not None:
            _EXT.prebuild_async(self.core, int(what), bool(avg))

    # ------------------------------------------------------------------ views (tests, the builder's cache tuples)
    def _info(self):
        if self.core is not None:
            return self.core.info()
        out = (C.c_longlong * 16)()
        check(_lib.load().mccnn_geometry_info(self.handle, out), "geometry_info")
        return list(out)

    def _view(self, owner_buf, addr, nbytes, dtype, shape):
        off = addr - owner_buf.data_ptr()
        return owner_buf[off:off + nbytes].view(dtype).view(shape)

    def _join(self):
        """A build issued on a side stream: whoever READS the arrays through tensor views does so on the current stream."""
        for g in (self, self.grid_owner):
            if g is not None and g.core is not None and g.buf is not None:
                g.core.join(g.buf)

    def grid(self):
        """(sortPts [n,3], sortBatchs [n,1], cellIndexs [B,nc,nc,nc,2], index_new_pos [n], inverse [n])"""
        self._join()
        i = self._info()
        ob = (self.grid_owner or self).buf
        n, nc, B = self.n, self.nc, self.B
        return (self._view(ob, i[0], n * 12, torch.float32, (n, 3)), self._view(ob, i[1], n * 4, torch.int32, (n, 1)),
                self._view(ob, i[2], B * nc ** 3 * 8, torch.int32, (B, nc, nc, nc, 2)),
                self._view(ob, i[3], n * 4, torch.int32, (n,)), self._view(ob, i[4], n * 4, torch.int32, (n,)))

    def neighbors(self):
        """(startIndexs [m,1], packedNeighs [E,2])"""
        e = self.edges()
        self._join()
        i = self._info()
        return (self._view(self.buf, i[5], self.m * 4, torch.int32, (self.m, 1)),
                self._view(self.buf, i[6], e * 8, torch.int32, (e, 2)))

    def pdfs(self):
        """[E,1]: the KDE of the list, or (a geometry built with pointPDF) the per-point density expanded over it"""
        e = self.edges()
        self._join()
        i = self._info()
        return self._view(self.buf, i[7], e * 4, torch.float32, (e, 1))

    def records(self):
        """(avg, records [E,4] f32) -- the per-edge records (delta, 1 / (pdf K)) the geometry holds, in edge order, and the
        `avg` flag they were made for; None when it holds none (not asked for, or MCCNN_DEBUG=kde_records=0)."""
        e = self.edges()
        self._join()
        if self.core is not None:
            avg, addr = self.core.records()
        else:
            p = C.c_void_p(0)
            avg = _lib.load().mccnn_geometry_records(self.handle, C.byref(p))
            addr = p.value or 0
        if avg < 0 or not addr:
            return None
        off = addr - self.buf.data_ptr()
        if off < 0 or off + e * 16 > self.buf.numel():
            return None   # (records in an attached buffer of a row plan, not the build's own)
        return int(avg), self._view(self.buf, addr, e * 16, torch.float32, (e, 4))

    def chosen_cap(self):
        """int32 [1] on the device: the cap the search ran with -- K*, the cap a budgeted search chose (a view of the
        geometry's own word, written by the build; never read back here), or without a budget the caller's maxNeighbors.
        Readable on the current stream."""
        if self.budget <= 0:
            return torch.full((1,), self.cap[0], dtype=torch.int32, device=self.buf.device)
        # (no wait for the edge total: the selection runs before the fill pass, so a list that outgrows its buffer and is
        # built again leaves the same K* in the word of either buffer, and the view keeps its buffer alive)
        self._join()
        if self.core is not None:
            addr = int(self.core.cap_addr())
        else:
            addr = int(_lib.load().mccnn_geometry_cap(self.handle) or 0)
        if not addr:
            raise _lib.MCCNNError("geometry: no cap word (built without a budget)")
        return self._view(self.buf, addr, 4, torch.int32, (1,))

    def point_density(self, window=None):
        """(density [n,1] f32, counts [n,1] i32) of the grid's sorted points at `window` (None: this geometry's own): the
        pair every point geometry over this grid and window shares -- the same tensors whichever of them is asked. Readable
        on the current stream."""
        w = float(self.window if window is None else window)
        pair = (self.grid_owner or self).pointPairs.get(w)
        if pair is None:
            raise KeyError("geometry: no per-point density at window %r over this grid" % (w,))
        if pair[2] is not None:
            pair[2].join()
        return pair[0], pair[1]


def _build_into(g, inPts, inBids, centres, cbids, mn, mx, B, nc, radius, scaleInv, window, usePDF, capacity, grid_from,
                side=-1, fork=False, background=False, after=None, maxNeighbors=0, sampleSeed=None, pointPDF=False, maxEdges=0,
                recordsAvg=None):
    n, m = inPts.shape[0], centres.shape[0]
    # per-edge records from the build's KDE: only lists whose PDFs come from it (MCCNN_DEBUG=kde_records=0: never)
    if recordsAvg is not None and not (_KDE_RECORDS and usePDF and not pointPDF):
        recordsAvg = None
    g.recordsAvg = None if recordsAvg is None else int(bool(recordsAvg))
    g.cap = (int(maxNeighbors), None if sampleSeed is None else int(sampleSeed))   # (a rebuild repeats them: _rebuild)
    g.budget = int(maxEdges)
    g.point, g.window = bool(pointPDF), float(window)
    pairs = (grid_from if grid_from is not None else g).pointPairs   # (the grid's owner keeps the densities)
    pair = pairs.get(g.window) if pointPDF else None
    if _EXT is not None:
        uses = g.core.uses if g.core is not None else 0
        g.core = _EXT.build_geometry(inPts, inBids, centres, cbids, mn, mx, B, nc, float(radius), bool(scaleInv), float(window),
                                     bool(usePDF), capacity, grid_from.core if grid_from is not None else None, side, fork,
                                     background, after, int(maxNeighbors), -1 if sampleSeed is None else int(sampleSeed),
                                     bool(pointPDF), pair[2] if pair is not None else None, int(maxEdges),
                                     -1 if g.recordsAvg is None else g.recordsAvg)
        if pointPDF and pair is None:
            pp = g.core.point
            pairs[g.window] = (pp.density, pp.counts, pp)
        g.core.uses = uses
        g.buf = g.core.buf
        g.grid_owner = grid_from
        g.n, g.m, g.nc, g.B, g.e_cap, g.e = n, m, nc, B, capacity, -1
        g.args = (inPts, inBids, centres, cbids, mn, mx, B, nc, radius, scaleInv, window, usePDF)
        return
    lib = _lib.load()
    dev = inPts.device
    with_grid = 0 if grid_from is not None else 1
    nbytes = lib.mccnn_geometry_bytes_budget(n, m, B, nc, capacity, with_grid, int(maxNeighbors), int(maxEdges))
    if nbytes == 0:
        raise _lib.MCCNNError("geometry: batch_size * num_cells^3 does not fit 32-bit keys")
    if g.handle is None:
        g.handle = lib.mccnn_geometry_create()
        if not g.handle:
            raise MemoryError("mccnn_geometry_create")
    if g.slot is None:
        g.slot = _slot()
    check(lib.mccnn_geometry_want_records(g.handle, -1 if g.recordsAvg is None else g.recordsAvg), "geometry_want_records")
    if g.recordsAvg is not None:   # (behind the geometry's own pieces, in the same buffer)
        nbytes += lib.mccnn_geometry_records_bytes(capacity)
    g.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    g.attached = []
    g.keep = (inPts, inBids, centres, cbids, mn, mx)
    g.grid_owner = grid_from
    g.n, g.m, g.nc, g.B, g.e_cap, g.e = n, m, nc, B, capacity, -1
    g.args = (inPts, inBids, centres, cbids, mn, mx, B, nc, radius, scaleInv, window, usePDF)
    cap = _NeighborCap(int(maxNeighbors), 0 if sampleSeed is None else 1, 0 if sampleSeed is None else int(sampleSeed))
    point = _PointPdf(None, None, 0)
    if pointPDF:   # (everything of this binding runs on the current stream: the density lies in stream order before its users)
        ready = pair is not None
        if not ready:
            pair = (torch.empty((n, 1), dtype=torch.float32, device=dev), torch.empty((n, 1), dtype=torch.int32, device=dev), None)
        point = _PointPdf(pair[0].data_ptr(), pair[1].data_ptr(), 1 if ready else 0)
    budget = _NeighborBudget(int(maxEdges))
    check(lib.mccnn_geometry_build_budget(g.handle, ptr(inPts), ptr(inBids), n, ptr(centres), ptr(cbids), m, ptr(mn), ptr(mx), B,
                                         nc, float(radius), int(bool(scaleInv)), float(window), int(bool(usePDF)), capacity,
                                         grid_from.handle if grid_from is not None else None, g.buf.data_ptr(), nbytes,
                                         g.slot.data_ptr(), stream_handle(), C.addressof(cap), C.addressof(point), C.addressof(budget)),
          "geometry_build")
    if pointPDF:
        pairs[g.window] = pair


def begin_batch():
    """Geometries requested until end_batch() that go to a side stream are issued as ONE batch -- one launch per kernel kind
    over all of them (mccnn_geometry_build_batch) -- on one side stream (torch extension only; otherwise a no-op)."""
    if _EXT is not None:
        _EXT.begin_geometry_batch()


def end_batch():
    if _EXT is not None:
        _EXT.end_geometry_batch()


def side_streams_available():
    """Geometry builds on side streams need the torch extension (events and streams live on its side)."""
    return _EXT is not None


def build_geometry(inPts, inBids, centres, cbids, mn, mx, B, nc, radius, scaleInv, window, usePDF, grid_from=None,
                   side=-1, fork=False, background=False, after=None, maxNeighbors=0, sampleSeed=None, pointPDF=False,
                   maxEdges=0, recordsAvg=None):
    """Enqueues grid + search + KDE of one convolution geometry; no host wait. nc: cells per axis
    (MCConvModule._num_cells). grid_from: a Geometry over the same points / radius whose grid is shared. side >= 0
    (torch extension only): the build runs on side stream `side` -- behind everything the current stream holds at the
    first call that says fork=True -- and the first layer that uses the geometry orders its stream behind it.
    after: the future of the ADOPTED prefetched hierarchy that every input of this build belongs to; a side-stream build
    then waits for that hierarchy only and takes its memory from its own stream's pool (torch_ext.cpp, Geo::own_pool).
    maxNeighbors > 0: the search keeps at most that many neighbours per centre (find_neighbors(maxNeighbors=), the same
    bytes); sampleSeed (needs a cap): the seed the capped search draws its stratified sample with, as the op takes it. The
    list then holds at most m * maxNeighbors rows: a capacity of that size cannot overflow, and the guess an uncapped list
    of the shape would get is used only where it is smaller.
    pointPDF (needs usePDF and no cap): the PDFs are the per-point density of (grid, window) expanded over the list --
    compute_pdf_points + expand_pdf of the op surface, the same bytes -- instead of the KDE of the list. The grid's owner keeps
    ONE (density, counts) pair per window (Geometry.point_density); the first build over a grid and window computes it
    right behind the grid, every later one, whatever its centres and stream, only expands it.
    maxEdges = B > 0 (with or without a cap of the caller's; not with pointPDF): the search picks, on the device, the largest
    cap K* whose list has at most B rows (find_neighbors(maxEdges=), the same bytes) -- Geometry.chosen_cap() is the device
    word it lands in. The list holds at most max(B, m) rows: the capacity is min(max(B, m), guess), and guesses of budgeted
    shapes are kept apart from those of every other shape.
    recordsAvg (None: no): the KDE of the build also leaves the per-edge records (delta, 1 / (pdf K)) the convolution kernels
    read, for layers whose useAVG is this flag -- behind the geometry's pieces, in its buffer (16 bytes per edge of the
    capacity). A one-input-feature combin layer over the geometry then reads them in both passes and neither evaluates nor
    keeps records of its own (mccnn_geometry_want_records). Without effect on lists without a KDE (usePDF=False, pointPDF)."""
    n, m = inPts.shape[0], centres.shape[0]
    if isinstance(maxEdges, bool) or not isinstance(maxEdges, int) or not 0 <= maxEdges < 2 ** 31:
        raise ValueError("build_geometry: maxEdges is an integer in [0, 2^31) (0 = no budget)")
    maxNeighbors = int(maxNeighbors)
    if maxNeighbors < 0 or (sampleSeed is not None and ((maxNeighbors == 0 and maxEdges == 0) or not 0 <= int(sampleSeed) < 2 ** 32)):
        raise ValueError("build_geometry: maxNeighbors >= 0; sampleSeed needs a cap or a budget and lies in [0, 2^32)")
    if pointPDF and (maxNeighbors > 0 or maxEdges > 0 or not usePDF):
        raise ValueError("build_geometry: pointPDF needs usePDF and an uncapped list (no cap, no budget)")
    gkey = (inPts.device.index, n, m, float(radius), int(B), bool(scaleInv))
    if maxNeighbors > 0:
        # (capped totals never shrink the guess of an uncapped geometry of the shape, or the reverse: the cap is a seventh
        # element of the key, which _edge_guess / _remember_edges carry into the key of the edges-per-centre table)
        gkey = gkey + (maxNeighbors,)
    if maxEdges > 0:   # (... and budgeted totals move the guesses of their own (cap, budget) alone)
        gkey = gkey[:6] + ((maxNeighbors, maxEdges),)
    g = Geometry()
    g.gkey = gkey
    if grid_from is not None and grid_from.grid_owner is not None:
        grid_from = grid_from.grid_owner
    capacity = _capacity_guess(gkey, m)
    if maxNeighbors > 0:
        capacity = max(1, min(m * maxNeighbors, capacity))
    if maxEdges > 0:   # (at max(B, m) rows the list cannot overflow)
        capacity = max(1, min(max(maxEdges, m), capacity))
    _build_into(g, inPts, inBids, centres, cbids, mn, mx, B, nc, radius, scaleInv, window, usePDF,
                capacity, grid_from, side if _EXT is not None else -1, fork, background,
                after if _EXT is not None else None, maxNeighbors, sampleSeed, pointPDF, maxEdges, recordsAvg)
    return g


_I0 = C.c_int
_LL = C.c_longlong


def _prepare(geo, feats, fin, fout, combin, bf16, backward, flags):
    """-> (ws bytes, saved bytes); attaches whatever the geometry lacks for this call."""
    lib = _lib.load()
    mask, edges = _I0(0), _I0(0)
    need = (_LL * 4)()
    wsb, svb = _LL(0), _LL(0)
    rc = lib.mccnn_conv_prepare(geo.handle, feats.data_ptr(), fin, fout, combin, bf16, backward, flags, C.byref(mask), need,
                                C.byref(wsb), C.byref(svb), C.byref(edges))
    if rc == E_CAPACITY:
        geo.edges()  # rebuilds with the exact size
        rc = lib.mccnn_conv_prepare(geo.handle, feats.data_ptr(), fin, fout, combin, bf16, backward, flags, C.byref(mask),
                                    need, C.byref(wsb), C.byref(svb), C.byref(edges))
    check(rc, "conv_prepare")
    if geo.e < 0:
        geo.e = edges.value
        _remember(geo.gkey, geo.m, geo.e)
    if mask.value:
        for k, bit in enumerate((NEED_PLAN_FWD, NEED_PLAN_TR, NEED_TLIST, NEED_RECORDS)):
            if mask.value & bit:
                t = torch.empty(max(int(need[k]), 256), dtype=torch.uint8, device=feats.device)
                check(lib.mccnn_geometry_attach(geo.handle, bit, t.data_ptr(), t.numel()), "geometry_attach")
                geo.attached.append(t)
    return wsb.value, svb.value


E_WORKSPACE = -4
_SIZES = {}   # (direction, fin, fout, combin, bf16, n, m) -> (scratch bytes, saved bytes) of the last call of this shape


class _Conv(torch.autograd.Function):
    """SpatialConv with sort_features folded in (MCConvModuleSrc:35-45,70-81) over a native Geometry. The calls are made
    OPTIMISTICALLY with the buffer sizes of the last call of the same shape; only when the library says something is
    missing (first batch of a shape, a longer list, a plan to attach) mccnn_conv_prepare is asked and the call repeated --
    nothing has been launched by then."""

    @staticmethod
    def forward(ctx, feats, w1, b1, w2, b2, w3, b3, geo, fout, combin, avg, deterministic):
        lib = _lib.load()
        fin = feats.shape[1]
        bf16 = 1 if feats.dtype == torch.bfloat16 else 0
        need_grad = feats.requires_grad or w1.requires_grad or w3.requires_grad or w2.requires_grad or b1.requires_grad \
            or b2.requires_grad or b3.requires_grad
        feats = _bf16_rows_aligned(feats)   # (no-op for f32 rows and aligned bf16 rows; both passes read the same tensor)
        flags = (CONV_KEEP_STATE if need_grad else 0) | (CONV_DETERMINISTIC if deterministic else 0)
        combin = 1 if combin else 0
        avg = 1 if avg else 0
        if fin == 1 and combin and lib.mccnn_conv_uses_records(geo.handle, fin, fout, combin, avg):
            flags |= CONV_READS_RECORDS   # the geometry holds this layer's per-edge records: read in both passes, kept by neither
        dev = feats.device
        out = torch.empty((geo.m, fout if combin else fin), dtype=feats.dtype, device=dev)
        skey = (flags & (CONV_KEEP_STATE | CONV_READS_RECORDS), fin, fout, combin, bf16, geo.n, geo.m)
        wsb, svb = _SIZES.get(skey, (0, -1))
        if svb < 0:
            wsb, svb = _prepare(geo, feats, fin, fout, combin, bf16, 0, flags)
            svb += svb // 16   # a little head room: the lists of a shape vary from batch to batch
        tried = False
        while True:
            saved = torch.empty(svb, dtype=torch.uint8, device=dev) if svb else None
            ws = _ws(wsb, dev)
            rc = lib.mccnn_conv_forward(geo.handle, feats.data_ptr(), fin, fout, combin, avg, bf16, flags, w1.data_ptr(),
                                        b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(), b3.data_ptr(),
                                        out.data_ptr(), ptr(saved), svb, ws.data_ptr(), ws.numel(), stream_handle())
            if rc == 0:
                break
            if rc not in (E_WORKSPACE, E_CAPACITY):
                check(rc, "conv_forward")
            w2_, s2_ = _prepare(geo, feats, fin, fout, combin, bf16, 0, flags)
            if s2_ <= svb and rc == E_WORKSPACE and ws.numel() >= w2_ and tried:
                check(rc, "conv_forward")  # the library asked twice for what it was given
            tried = True
            wsb, svb = w2_, s2_ + s2_ // 16
        if geo.e < 0:
            geo.e = lib.mccnn_geometry_edges(geo.handle, 0)
            _remember(geo.gkey, geo.m, geo.e)
        if len(_SIZES) > 1024:
            _SIZES.clear()
        _SIZES[skey] = (wsb, svb)
        if need_grad:
            ctx.save_for_backward(feats, w1, b1, w2, b2, w3, b3)
            ctx.saved_buf = saved
            ctx.geo = geo
            ctx.attrs = (fin, fout, combin, avg, bf16, flags)
        return out

    @staticmethod
    def backward(ctx, outGrad):
        feats, w1, b1, w2, b2, w3, b3 = ctx.saved_tensors
        geo, saved = ctx.geo, ctx.saved_buf
        fin, fout, combin, avg, bf16, flags = ctx.attrs
        if geo.uses > 1:
            # several layers share this neighbour list: its transposed form is built once and the feature gradient of
            # combin layers with 2..4 input features is gathered through it in a fixed order (bit-reproducible) instead
            # of added with float atomics; a bare single call keeps the atomics (the list would cost more than they do)
            flags |= CONV_DETERMINISTIC
        lib = _lib.load()
        og = outGrad if outGrad.is_contiguous() else outGrad.contiguous()
        if og.dtype != feats.dtype:
            og = og.to(feats.dtype)
        og = _bf16_rows_aligned(og)
        dev = feats.device
        fg = torch.empty_like(feats)
        # the six MLP gradients: consecutive slices of ONE buffer in the order the builder creates the variables (a
        # data-parallel step all-reduces that buffer as it is, dist.GradBucket)
        n1, n2, n3, n4, n5, n6 = w1.numel(), b1.numel(), w2.numel(), b2.numel(), w3.numel(), b3.numel()
        gflat = torch.empty(n1 + n2 + n3 + n4 + n5 + n6, dtype=torch.float32, device=dev)
        dw1, db1, dw2, db2, dw3, db3 = gflat.split((n1, n2, n3, n4, n5, n6))
        base = gflat.data_ptr()
        skey = (2, flags & CONV_DETERMINISTIC, fin, fout, combin, bf16, geo.n, geo.m)   # (deterministic and atomic backward passes differ in scratch)
        wsb = _SIZES.get(skey, (-1, 0))[0]
        if wsb < 0:
            wsb, _ = _prepare(geo, feats, fin, fout, combin, bf16, 1, flags)
        svn = saved.numel() if saved is not None else 0
        tried = False
        while True:
            ws = _ws(wsb, dev)
            rc = lib.mccnn_conv_backward(geo.handle, feats.data_ptr(), ptr(saved), svn, og.data_ptr(), fin, fout, combin, avg,
                                         bf16, flags, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), w3.data_ptr(),
                                         b3.data_ptr(), fg.data_ptr(), base, base + 4 * n1, base + 4 * (n1 + n2),
                                         base + 4 * (n1 + n2 + n3), base + 4 * (n1 + n2 + n3 + n4),
                                         base + 4 * (n1 + n2 + n3 + n4 + n5), ws.data_ptr(), ws.numel(), stream_handle())
            if rc == 0:
                break
            if rc not in (E_WORKSPACE, E_CAPACITY):
                check(rc, "conv_backward")
            w2_, _ = _prepare(geo, feats, fin, fout, combin, bf16, 1, flags)
            if tried and ws.numel() >= w2_:
                check(rc, "conv_backward")
            tried = True
            wsb = w2_
        _SIZES[skey] = (wsb, 0)
        return (fg, dw1.view_as(w1), db1, dw2.view_as(w2), db2.view_as(b2), dw3.view_as(w3), db3.view_as(b3),
                None, None, None, None, None)


def conv(geo, feats, w1, b1, w2, b2, w3, b3, numOutFeatures, combin, avg, deterministic=False):
    """One MC convolution over `geo`: feats are the rows of the UNSORTED input points ([n, Fin] f32, or bf16 for
    depth-wise layers); the kernel-MLP tensors in any shape over the reference's flat layout."""
    core = geo.core
    if core is not None:
        core.uses = geo.uses
        try:
            out = _EXT.conv(core, feats, w1, b1, w2, b2, w3, b3, numOutFeatures, bool(combin), bool(avg), bool(deterministic))
        except _EXT.CapacityError:
            geo.edges()   # the list did not fit the guess (first batch of a shape): exact rebuild, then the layer
            geo.core.uses = geo.uses
            out = _EXT.conv(geo.core, feats, w1, b1, w2, b2, w3, b3, numOutFeatures, bool(combin), bool(avg), bool(deterministic))
        if geo.e < 0:
            geo.e = geo.core.e
            _remember(geo.gkey, geo.m, geo.e)
        return out
    return _Conv.apply(feats, w1, b1, w2, b2, w3, b3, geo, numOutFeatures, combin, avg, deterministic)


# ---------------------------------------------------------------------------------------------
# The dense ops (dense_glue.py), each in two steps: X(...) = _X_run(*M._X_args(...)). M._X_args is the op's argument rule,
# the only one there is; _X_run takes what the rule returns to the extension when that is loaded, to the ctypes form
# (M._X_run) otherwise -- the same library calls either way, so the same bytes. A caller that has run the rule itself (the
# gates of MCNetworkUtils) calls _X_run.
def _out_flag(outDtype):
    return -1 if outDtype is None else int(outDtype == torch.bfloat16)


def _bn_act_run(x, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale):
    if _EXT is None:
        return M._bn_act_run(x, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale)
    return _EXT.bn_relu_drop(x, gamma, beta, movingMean, movingVar, bool(training), bool(relu), thr, scale, seed,
                             float(momentum), float(epsilon), _out_flag(outDtype))


def bn_relu_drop(x, gamma, beta, movingMean, movingVar, training, relu=True, keepProb=None, seed=0, momentum=0.99,
                 epsilon=1e-3, outDtype=None):
    """The dense glue as one op, y = drop(act(bn(x))) (dense_glue.bn_relu_dropout: its definition, checks and errors):
    one Python -> C++ call forward and an autograd node on the C++ side when the extension is loaded, the ctypes op
    otherwise -- the same library calls either way, so the same bytes. x: float32 or bfloat16 rows; outDtype: y's type
    (None: x's)."""
    return _bn_act_run(x, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype,
                       *M._bn_act_args(x, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, training=training))


def _bn_cat_run(xs, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale):
    if _EXT is None:
        return M._bn_cat_run(xs, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale)
    return _EXT.bn_relu_drop_cat(list(xs), gamma, beta, movingMean, movingVar, bool(training), bool(relu), thr, scale, seed,
                                 float(momentum), float(epsilon), _out_flag(outDtype))


def bn_relu_drop_cat(xs, gamma, beta, movingMean, movingVar, training, relu=True, keepProb=None, seed=0, momentum=0.99,
                     epsilon=1e-3, outDtype=None):
    """The dense glue over torch.cat(xs, 1) as one op that reads the segments where they are
    (dense_glue.bn_relu_dropout_cat: its definition, checks and errors): one Python -> C++ call forward and an autograd
    node on the C++ side (BnCatBackward) when the extension is loaded, the ctypes op otherwise -- the same library calls
    either way, so the same bytes. A segment that does not require a gradient gets None."""
    return _bn_cat_run(xs, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype,
                       *M._bn_cat_args(xs, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, training=training))


_EXT_SYNC_STAGES = None if _EXT is None else (_EXT.bn_sync_stats, _EXT.bn_sync_apply, _EXT.bn_sync_bwd_sums, _EXT.bn_sync_bwd_dx)


def _bn_sync_run(*checked):
    return M._bn_sync_run(*checked, stages=_EXT_SYNC_STAGES or M._BN_SYNC_STAGES)


def bn_relu_drop_sync(x, gamma, beta, movingMean, movingVar, relu=True, keepProb=None, seed=0, momentum=0.99, epsilon=1e-3,
                      outDtype=None, group=None):
    """The training form of the dense glue with batch statistics over the rows of all ranks of `group`
    (dense_glue.bn_relu_dropout_sync: its definition, checks and errors). The autograd node is that module's either way
    (the collectives between the stages are torch.distributed's); with the extension loaded its four stages are the
    extension's calls, with the ctypes ones otherwise -- the same library calls, so the same bytes."""
    return _bn_sync_run(x, gamma, beta, movingMean, movingVar, relu, seed, momentum, epsilon, outDtype, group,
                        *M._bn_act_args(x, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, sync=True, group=group))


def _linear_bn_run(x, w, b, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype, thr, scale):
    if _EXT is None:
        return M._linear_bn_run(x, w, b, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype,
                                thr, scale)
    return _EXT.linear_bn_relu_drop(x, w, b, gamma, beta, movingMean, movingVar, bool(training), bool(relu), thr, scale, seed,
                                    float(momentum), float(epsilon), _out_flag(outDtype))


def linear_bn_relu_drop(x, w, b, gamma, beta, movingMean, movingVar, training, relu=True, keepProb=None, seed=0, momentum=0.99,
                        epsilon=1e-3, outDtype=None):
    """A linear layer and the dense glue behind it as one op, y = drop(act(bn(x @ w + b)))
    (dense_glue.linear_bn_relu_dropout: its definition, checks and errors): one Python -> C++ call forward and an
    autograd node on the C++ side when the extension is loaded, the ctypes op otherwise -- the same library calls either
    way, so the same bytes."""
    return _linear_bn_run(x, w, b, gamma, beta, movingMean, movingVar, training, relu, seed, momentum, epsilon, outDtype,
                          *M._linear_bn_args(x, w, b, gamma, beta, movingMean, movingVar, keepProb, seed, outDtype, training=training))


def _linear_xent_run(*checked):
    return (M._linear_xent_run if _EXT is None else _EXT.linear_softmax_xent)(*checked)


def linear_softmax_xent(x, w, b, labels, weights=None, wantLogits=False):
    """The last linear layer and the softmax cross-entropy behind it as one op -> (loss, pred, meta, logits or None)
    (dense_glue.linear_softmax_xent: its definition, checks and errors): one Python -> C++ call forward and an autograd
    node on the C++ side (LinearXentBackward) when the extension is loaded, the ctypes op otherwise -- the same library
    calls either way, so the same bytes."""
    return _linear_xent_run(*M._linear_xent_args(x, w, b, labels, weights, wantLogits))


def _cosine_loss_run(*checked):
    return (M._cosine_loss_run if _EXT is None else _EXT.cosine_distance_loss)(*checked)


def cosine_distance_loss(pred, target, weights=None):
    """The cosine-distance loss of normal estimation as one op -> (loss, sums, meta) (dense_glue.cosine_distance_loss: its
    definition, checks and errors): one Python -> C++ call forward and an autograd node on the C++ side (CosineLossBackward)
    when the extension is loaded, the ctypes op otherwise -- the same library calls either way, so the same bytes."""
    return _cosine_loss_run(*M._cosine_loss_args(pred, target, weights))


def _seg_counts_run(*checked):
    return (M._seg_counts_run if _EXT is None else _EXT.segmentation_counts)(*checked)


def segmentation_counts(pred, labels, numClasses, batchIds=None, numClouds=1, weights=None, ignoreLabel=-1, out=None):
    """The counts behind the IoU of segmentation -> int64 (numClouds, numClasses, 3) (dense_glue.segmentation_counts: its
    definition, checks and errors): one Python -> C++ call on the current stream when the extension is loaded, the ctypes op
    otherwise -- the same library call either way, so the same bytes. A plain function: nothing is differentiable."""
    return _seg_counts_run(*M._seg_counts_args(pred, labels, numClasses, batchIds, numClouds, weights, ignoreLabel, out))


def _voxel_counts_run(*checked):
    if _EXT is None:
        return M._voxel_counts_run(*checked)
    points, numClasses = checked[0], checked[3]
    return _EXT.voxel_counts(*checked, M._voxel_ws(points.shape[0], numClasses, points.device) if points.shape[0] else None)


def voxel_counts(points, pred, labels, numClasses, batchIds=None, numClouds=1, aabbMin=None, resolution=0.05, ignoreLabel=-1,
                 maxIgnoreShare=0.3, out=None, dropped=None):
    """The counts behind ScanNet's voxel accuracy -> int64 (numClouds, numClasses, 2) (dense_glue.voxel_counts: its
    definition, checks, errors and its table): one Python -> C++ call on the current stream when the extension is loaded, the
    ctypes op otherwise -- the same library call either way, so the same bytes. A plain function: nothing is differentiable."""
    return _voxel_counts_run(*M._voxel_counts_args(points, pred, labels, numClasses, batchIds, numClouds, aabbMin, resolution,
                                                   ignoreLabel, maxIgnoreShare, out, dropped))


