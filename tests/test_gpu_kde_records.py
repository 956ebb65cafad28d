"""Per-edge records written by the KDE of a geometry's build (mccnn_geometry_want_records; neighbors.hip pdf_rows_mfma<W, true>)
at the level of the C-ABI: the records are the bytes of mccnn_edge_records over the finished list and its PDFs, and the PDFs,
the list and the row starts are the bytes of a build that was not asked for records (the code path of
MCCNN_DEBUG=kde_records=0). Lists: rows of every length around the tile sizes under both KDE kernels, one row beyond the
planes of a wave (pdf_row_long / the pooled planes), a pooling list with empty rows, two ragged clouds, a capped list; both
`avg` flags and both radius modes; and the batch form against the single chains."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import make_cloud

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 15, 16, 17, 63, 64, 65, 191, 192, 193)   # around the 16-point tiles, the 64 lanes and the 192-point planes
LONG = 800                                            # > 4 x 192: beyond the pooled planes of the 4-wave kernel
WINDOW = 0.2


def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _blobs(filler):
    """One tight blob (diameter < 0.02) per row length, 0.5 apart: at radius 0.1 every point's row is its blob. filler: 17 576
    isolated points on a 0.25 lattice behind them -- rows of length 1 that lift the list over the 16 384 rows from which the KDE
    takes four waves per workgroup and four rows per wave."""
    rng = np.random.default_rng(3)
    parts = []
    for i, k in enumerate(ROWS + (LONG,)):
        c = np.array([0.5 * i, 0.0, 0.0], dtype=np.float32)
        parts.append(c + (rng.random((k, 3), dtype=np.float32) - 0.5) * 0.01)
    if filler:
        ax = np.arange(26, dtype=np.float32) * 0.25
        g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
        parts.append(g + np.array([0.0, 1.0, 0.0], dtype=np.float32))
    pts = np.concatenate(parts).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    return pts, np.zeros((len(pts), 1), dtype=np.int32)


def _case(name):
    """-> points, ids, centres, ids, B, radius (absolute units), cap"""
    if name in ("blobs4", "blobs16"):
        p, b = _blobs(name == "blobs4")
        return p, b, p, b, 1, 0.1, 0
    if name == "pool":
        p, b = make_cloud(900, 3, 33, "clustered", True)
        rng = np.random.default_rng(10)
        sel = np.sort(rng.choice(len(p), len(p) // 7, replace=False))
        far = np.full((5, 3), 40.0, dtype=np.float32) + rng.random((5, 3), dtype=np.float32)   # no neighbours at all
        c = np.concatenate([p[sel][:50], far[:2], p[sel][50:], far[2:]]).astype(np.float32)
        cb = np.concatenate([b[sel][:50], b[:2] * 0, b[sel][50:], b[:3] * 0]).astype(np.int32)
        return p, b, c, cb, 3, 0.3, 0
    p, b = make_cloud(1500, 2, 33, "clustered", True)   # "ragged2" / "capped"
    return p, b, p, b, 2, 0.15, (8 if name == "capped" else 0)


class _Cap(C.Structure):
    _fields_ = [("max_neighbors", C.c_int), ("sampled", C.c_int), ("seed", C.c_uint)]


class _Req(C.Structure):
    _fields_ = [("geometry", C.c_void_p), ("pts", C.c_void_p), ("batch_ids", C.c_void_p), ("n", C.c_int),
                ("centres", C.c_void_p), ("centre_batch_ids", C.c_void_p), ("m", C.c_int), ("aabb_min", C.c_void_p),
                ("aabb_max", C.c_void_p), ("batch_size", C.c_int), ("num_cells", C.c_int), ("radius", C.c_float),
                ("scale_inv", C.c_int), ("window", C.c_float), ("use_pdf", C.c_int), ("e_capacity", C.c_int),
                ("grid_from", C.c_void_p), ("buffer", C.c_void_p), ("buffer_bytes", C.c_size_t), ("total_host", C.c_void_p)]


def _lib():
    from mccnn_amd import _lib as L
    lib = L.load()
    lib.mccnn_geometry_create.restype = C.c_void_p
    return lib


class _Geo:
    """One geometry through the C-ABI: inputs on the device, its buffer, the request record of the batch form."""

    def __init__(self, mc, name, scale_inv, avg, e_cap=None):
        import torch
        lib = _lib()
        p, b, c, cb, self.B, radius, self.cap = _case(name)
        self.P, self.Bi = _t(p), _t(b)
        same = c is p
        self.Cn, self.Cb = (self.P, self.Bi) if same else (_t(c), _t(cb))
        self.n, self.m, self.scale_inv, self.avg = len(p), len(c), scale_inv, avg
        self.mn, self.mx = mc.compute_aabb(self.P, self.Bi, self.B, scale_inv)
        if scale_inv:   # the same balls in relative units (the clouds of a batch share one box here: aabb of the whole batch)
            ext = float((self.mx - self.mn).max())
            radius = radius / ext
        self.radius = radius
        self.nc = mc._num_cells(self.mn, self.mx, self.B, radius, scale_inv)
        self.e_cap = e_cap if e_cap is not None else 60 * self.m + LONG * LONG + 200000
        self.h = lib.mccnn_geometry_create()
        self.slot = torch.full((1,), -1, dtype=torch.int32).pin_memory()
        self.buf = None

    def request(self, records):
        import torch
        from mccnn_amd._lib import ptr, check
        lib = _lib()
        lib.mccnn_geometry_records_bytes.restype = C.c_size_t
        nbytes = lib.mccnn_geometry_bytes_capped(self.n, self.m, self.B, self.nc, self.e_cap, 1, self.cap)
        check(lib.mccnn_geometry_want_records(C.c_void_p(self.h), self.avg if records else -1), "want_records")
        if records:
            nbytes += lib.mccnn_geometry_records_bytes(self.e_cap)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        return _Req(self.h, ptr(self.P), ptr(self.Bi), self.n, ptr(self.Cn), ptr(self.Cb), self.m, ptr(self.mn), ptr(self.mx), self.B,
                    self.nc, self.radius, 1 if self.scale_inv else 0, WINDOW, 1, self.e_cap, None, self.buf.data_ptr(), nbytes,
                    self.slot.data_ptr())

    def build(self, records):
        import torch
        from mccnn_amd._lib import check
        lib = _lib()
        q = self.request(records)
        cap = _Cap(self.cap, 0, 0)
        lib.mccnn_geometry_build_capped.argtypes = None
        check(lib.mccnn_geometry_build_capped(C.c_void_p(q.geometry), C.c_void_p(q.pts), C.c_void_p(q.batch_ids), q.n, C.c_void_p(q.centres),
                                              C.c_void_p(q.centre_batch_ids), q.m, C.c_void_p(q.aabb_min), C.c_void_p(q.aabb_max),
                                              q.batch_size, q.num_cells, C.c_float(q.radius), q.scale_inv, C.c_float(q.window), q.use_pdf,
                                              q.e_capacity, None, C.c_void_p(q.buffer), C.c_size_t(q.buffer_bytes), C.c_void_p(q.total_host),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cap)), "geometry_build")
        return self.read()

    def read(self):
        """-> dict of host copies: e, start, packed, pdfs (raw int32 words), rec (raw words or None), rec_avg"""
        import torch
        from mccnn_amd._lib import check
        lib = _lib()
        torch.cuda.synchronize()
        e = int(self.slot[0])
        assert 0 <= e <= self.e_cap, (e, self.e_cap)
        info = (C.c_longlong * 16)()
        check(lib.mccnn_geometry_info(C.c_void_p(self.h), info), "geometry_info")

        def view(addr, nbytes):
            off = addr - self.buf.data_ptr()
            assert 0 <= off and off + nbytes <= self.buf.numel()
            return self.buf[off:off + nbytes].view(torch.int32)
        p = C.c_void_p(0)
        lib.mccnn_geometry_records.argtypes = None
        avg = lib.mccnn_geometry_records(C.c_void_p(self.h), C.byref(p))
        out = dict(e=e, start=view(info[5], self.m * 4), packed=view(info[6], e * 8), pdfs=view(info[7], e * 4), rec_avg=avg,
                   rec=view(p.value, e * 16) if (avg >= 0 and p.value) else None,
                   sP=view(info[0], self.n * 12), sB=view(info[1], self.n * 4))
        return out

    def reference_records(self, got):
        """mccnn_edge_records over the arrays of the built geometry"""
        import torch
        from mccnn_amd._lib import ptr, check
        lib = _lib()
        ref = torch.full((max(got["e"], 1) * 4,), 0x7fc00000, dtype=torch.int32, device="cuda")
        check(lib.mccnn_edge_records(ptr(got["sP"]), ptr(got["sB"]), ptr(got["pdfs"]), ptr(self.Cn), ptr(got["start"]), ptr(got["packed"]),
                                     ptr(self.mn), ptr(self.mx), self.n, self.m, got["e"], self.B, self.radius,
                                     1 if self.scale_inv else 0, self.avg, ptr(ref), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "edge_records")
        torch.cuda.synchronize()
        return ref[:got["e"] * 4]

    def close(self):
        _lib().mccnn_geometry_destroy(C.c_void_p(self.h))
        self.h = None


def _row_lengths(d, m):
    st = d["start"].cpu().numpy().astype(np.int64)
    return np.diff(np.concatenate([st, [d["e"]]]))


def _bytes_equal(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _check_property(name, g, d):
    k = _row_lengths(d, g.m)
    assert d["e"] > 0 and int(k.sum()) == d["e"]
    if name in ("blobs4", "blobs16"):
        for L in ROWS + (LONG,):   # every blob is one row length, once per point of the blob
            assert int((k == L).sum()) >= L, (L, int((k == L).sum()))
        assert k.max() == LONG > 4 * 192
        # 4 waves x 4 rows from 16 384 rows on (the long row: pdf_row_long); below, 16 waves (the long row: pooled planes)
        assert (g.m >= 16384) == (name == "blobs4") and LONG <= 16 * 192
    elif name == "pool":
        assert g.m != g.n and int((k == 0).sum()) >= 5
    elif name == "ragged2":
        n0 = int((g.Bi == 0).sum())
        assert g.B == 2 and 0 < n0 < g.n and n0 != g.n - n0
    elif name == "capped":
        assert k.max() == g.cap and int((k == g.cap).sum()) > 100   # the cap bites


CASES = [   # list, relative radius, avg
    ("blobs4", False, True), ("blobs4", True, False), ("blobs16", False, False), ("blobs16", True, True),
    ("pool", True, True), ("pool", False, False), ("ragged2", True, True), ("ragged2", False, False), ("capped", True, True),
]


@pytest.mark.parametrize("name,scale_inv,avg", CASES)
def test_kde_records_are_the_bytes_of_edge_records(mc, name, scale_inv, avg):
    plain = _Geo(mc, name, scale_inv, int(avg))
    with_rec = _Geo(mc, name, scale_inv, int(avg))
    try:
        a = plain.build(False)
        assert a["rec"] is None and a["rec_avg"] == -1
        _check_property(name, plain, a)
        b = with_rec.build(True)
        assert b["e"] == a["e"]
        for key in ("start", "packed", "pdfs"):      # the list and the PDFs: the bytes of a build without records
            assert _bytes_equal(a[key], b[key]), key
        assert b["rec_avg"] == int(avg) and b["rec"] is not None
        ref = with_rec.reference_records(b)
        assert _bytes_equal(b["rec"], ref)
        # (the query the layers ask: a one-input-feature combin layer of this `avg` reads them, nothing else does)
        lib = _lib()
        assert lib.mccnn_conv_uses_records(C.c_void_p(with_rec.h), 1, 64, 1, int(avg)) == 1
        assert lib.mccnn_conv_uses_records(C.c_void_p(with_rec.h), 1, 64, 1, 1 - int(avg)) == 0
        assert lib.mccnn_conv_uses_records(C.c_void_p(with_rec.h), 3, 8, 1, int(avg)) == 0
        assert lib.mccnn_conv_uses_records(C.c_void_p(plain.h), 1, 64, 1, int(avg)) == 0
    finally:
        plain.close()
        with_rec.close()


def test_a_buffer_without_room_builds_without_records(mc):
    """The request is an offer: a build whose buffer has the plain size ignores it."""
    import torch
    from mccnn_amd._lib import check
    lib = _lib()
    g = _Geo(mc, "ragged2", True, 1)
    try:
        q = g.request(False)
        check(lib.mccnn_geometry_want_records(C.c_void_p(g.h), 1), "want_records")
        lib.mccnn_geometry_build.argtypes = None
        check(lib.mccnn_geometry_build(C.c_void_p(q.geometry), C.c_void_p(q.pts), C.c_void_p(q.batch_ids), q.n, C.c_void_p(q.centres),
                                       C.c_void_p(q.centre_batch_ids), q.m, C.c_void_p(q.aabb_min), C.c_void_p(q.aabb_max), q.batch_size,
                                       q.num_cells, C.c_float(q.radius), q.scale_inv, C.c_float(q.window), q.use_pdf, q.e_capacity, None,
                                       C.c_void_p(q.buffer), C.c_size_t(q.buffer_bytes), C.c_void_p(q.total_host),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "geometry_build")
        d = g.read()
        assert d["e"] > 0 and d["rec"] is None and d["rec_avg"] == -1
    finally:
        g.close()


def test_batch_form_gives_the_bytes_of_the_single_chains(mc):
    """mccnn_geometry_build_batch over three of the lists (both `avg` flags) and one without a request: lists, PDFs and records
    are the bytes of the single chains. A fourth list with records, the many-row one: in a batch it runs four rows per wave
    under the 16-wave kernel and its 800-point row in the pooled planes (Gram tiles), where its own chain walks that row with
    the subtract-first loop -- other PDF bits for that one row, as before the records; its records are held against
    mccnn_edge_records over the batch's own arrays, its other rows against the single chain."""
    import torch
    from mccnn_amd._lib import check
    lib = _lib()
    specs = [("pool", True, 1, True), ("ragged2", True, 0, True), ("blobs16", False, 1, True), ("blobs16", True, 0, False),
             ("blobs4", False, 1, True)]
    single, batch = [], []
    try:
        for name, si, avg, rec in specs:
            g = _Geo(mc, name, si, avg)
            batch.append(g)   # (closed below with the rest)
            single.append(g.build(rec))
        singles_geo, batch = batch, [_Geo(mc, name, si, avg) for name, si, avg, rec in specs]
        reqs = (_Req * len(batch))()
        for k, (g, (_, _, _, rec)) in enumerate(zip(batch, specs)):
            reqs[k] = g.request(rec)
        check(lib.mccnn_geometry_build_batch(C.byref(reqs), len(batch), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "geometry_build_batch")
        for g, s, (name, _, avg, rec) in zip(batch, single, specs):
            d = g.read()
            assert d["e"] == s["e"], name
            for key in ("start", "packed"):
                assert _bytes_equal(d[key], s[key]), (name, key)
            if name == "blobs4":
                k = torch.from_numpy(_row_lengths(d, g.m)).cuda()
                short = torch.repeat_interleave(k <= 192, k)            # per edge: its row fits the planes of a wave
                assert int((~short).sum()) == LONG * LONG + 193 * 193   # (the rows set aside for the workgroup's pooled planes)
                assert torch.equal(d["pdfs"][short], s["pdfs"][short])
                assert d["rec_avg"] == avg and _bytes_equal(d["rec"], g.reference_records(d))
                assert torch.equal(d["rec"].view(-1, 4)[short], s["rec"].view(-1, 4)[short])
                continue
            assert _bytes_equal(d["pdfs"], s["pdfs"]), name
            if rec:
                assert d["rec_avg"] == avg and _bytes_equal(d["rec"], s["rec"]), name
            else:
                assert d["rec"] is None and d["rec_avg"] == -1
    finally:
        for g in batch + (singles_geo if "singles_geo" in locals() else []):
            g.close()


_OFF_SCRIPT = """
import ctypes as C, sys
sys.path.insert(0, %r)
import mccnn_amd.MCConvModule as M
import tests.test_gpu_kde_records as T
g = T._Geo(M, "ragged2", True, 1)
d = g.build(True)
print("RESULT", d["e"], d["rec_avg"], d["rec"] is None, int(d["pdfs"].long().sum()))
"""


def test_debug_key_switches_the_records_off(mc):
    """MCCNN_DEBUG=kde_records=0 (read once per process: a child process): a build that asks for records gets none, and its
    PDFs are those of this process's build."""
    g = _Geo(mc, "ragged2", True, 1)
    try:
        d = g.build(True)
        want = (d["e"], int(d["pdfs"].long().sum()))
        assert d["rec"] is not None
    finally:
        g.close()
    env = dict(os.environ, MCCNN_DEBUG="kde_records=0")
    r = subprocess.run([sys.executable, "-c", _OFF_SCRIPT % ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert (int(line[1]), int(line[4])) == want and line[2] == "-1" and line[3] == "True", line
