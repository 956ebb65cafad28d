"""The three kernels that walk the 27-cell window (csrc/cell_window.h: the neighbour search, the per-point density, its
position gradients) pinned byte for byte: SHA-256 digests of their raw output buffers, recorded on an MI355X at the commit
named in the header of tests/golden/window_pinned.json, before the three kernels shared their window walk. The test
recomputes the digests and asserts equality -- no tolerance, and no comparison of the code under test with itself.

Per case: find_neighbors (start indices, packed list) plain, capped (maxNeighbors=5) and sampled (maxNeighbors=5, one fixed
sampleSeed); compute_pdf_points (density, counts); mccnn_compute_pdf_points_bwd for a seeded density_grad (dpts, and dradius
where scaleInv).

Which case supplies which path (test_the_inputs_reach_every_path counts them on the CPU, over the oracle's grid):
  * a window of more than 256 candidates -- a second LDS segment in all three kernels: mid_windows (257 .. 512), big_windows;
  * a window of more than 512 candidates -- the search's fill pass leaves the saved-mask path and searches again: big_windows
    (1057 of its 3000 windows; mixed has 70 windows of 257 .. 512, many_centres none above 256);
  * several members of one wave in one cell, and a wave whose members span two cells: the group cases -- 8201 / 16390 /
    32771 members put 2 / 4 / 8 on a wave (the gradients: 2 / 4 / 4), each N leaves the last wave's group part empty; the
    four geometries run one member per wave;
  * a cloud id without points: the group cases, whose batch size is 2 while every point has id 0 (an empty box: FLT_MAX,
    -FLT_MAX; under the relative radius of group_16390 its extent never meets a point);
  * centres that are not the points, rows without hits, two clouds: mixed, many_centres."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import neighbor_cap_ref as geo
from tests import point_pdf_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_pinned.json")
WINDOW = 0.25
CAP = 5
SAMPLE_SEED = 20231
GROUPS = {"group_8201": (8201, 0.08, False), "group_16390": (16390, 0.0625, True), "group_32771": (32771, 0.05, False)}
CASES = list(geo.GEOMETRIES) + list(GROUPS)


def inputs(name):
    """-> dict(pts, bids, centres (None: the sorted points themselves), cbids, B, radius, scaleInv)."""
    if name in geo.GEOMETRIES:
        return geo.GEOMETRIES[name]()
    n, radius, scaleInv = GROUPS[name]
    pts = np.random.default_rng(n).random((n, 3), dtype=np.float32)   # (the clouds of test_every_group_size)
    return dict(pts=pts, bids=np.zeros((n, 1), np.int32), centres=None, cbids=None, B=2, radius=radius, scaleInv=scaleInv)


def grad_seed(name):
    return sum(map(ord, name))


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _digest(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def run_case(mc, name):
    """Every pinned output of one case on the GPU -> {output name: {shape, dtype, sha256}}."""
    import torch
    from mccnn_amd import _lib as L
    g = inputs(name)
    B, radius, si = g["B"], g["radius"], g["scaleInv"]
    P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
    mn, mx = mc.compute_aabb(P, Bi, B, si)
    sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, B, radius, si)
    if g["centres"] is None:
        C, Cb = sP.clone(), sB.clone()
    else:
        C, Cb = _wrap(g["centres"]), _wrap(g["cbids"])
    out = {}
    for tag, kw in (("plain", {}), ("capped", dict(maxNeighbors=CAP)), ("sampled", dict(maxNeighbors=CAP, sampleSeed=SAMPLE_SEED))):
        st, pk = mc.find_neighbors(C, Cb, sP, cells, mn, mx, radius, B, si, **kw)
        out["start_" + tag], out["packed_" + tag] = _digest(st), _digest(pk)
    density, counts = mc.compute_pdf_points(sP, sB, cells, mn, mx, WINDOW, radius, B, si)
    out["density"], out["counts"] = _digest(density), _digest(counts)
    n = sP.shape[0]
    gd = _wrap(np.random.default_rng(grad_seed(name)).random(n, dtype=np.float32))
    lib = L.load()
    dp = torch.full((n, 3), float("nan"), device="cuda")
    dR = torch.full((B,), float("nan"), device="cuda") if si else None
    ws = torch.empty(lib.mccnn_compute_pdf_points_bwd_workspace_bytes(n, B), dtype=torch.uint8, device="cuda")
    L.check(lib.mccnn_compute_pdf_points_bwd(L.ptr(sP), L.ptr(sB), n, L.ptr(cells), L.ptr(mn), L.ptr(mx), B, cells.shape[1], WINDOW,
                                             radius, int(si), L.ptr(gd), L.ptr(dp), L.ptr(dR) if si else None, L.ptr(ws), ws.numel(),
                                             L.stream_handle()), "compute_pdf_points_bwd")
    torch.cuda.synchronize()
    out["dpts"] = _digest(dp)
    if si:
        out["dradius"] = _digest(dR)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_the_window_kernels_give_the_recorded_bytes(mc, name):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["window"] == WINDOW and gold["maxNeighbors"] == CAP and gold["sampleSeed"] == SAMPLE_SEED
    want = gold["cases"][name]
    assert want["grad_seed"] == grad_seed(name)
    got = run_case(mc, name)
    assert sorted(got) == sorted(want["outputs"])
    diff = [k for k in sorted(got) if got[k] != want["outputs"][k]]
    for k in diff:
        print("%s %s: got %s, recorded %s" % (name, k, got[k], want["outputs"][k]))
    assert not diff, "%s: outputs that are not the recorded bytes: %s" % (name, diff)


def _census(oracle, name):
    """Window sizes seen by the search (its centres) and by the sweeps (the sorted points), and the cells of the sorted points."""
    g = inputs(name)
    mn, mx, sP, sB, cells, idx = ref.sorted_grid(oracle, g["pts"], g["bids"], g["B"], g["radius"], g["scaleInv"])
    r = dict(cellIndexs=cells, aabbMin=mn, aabbMax=mx)
    own = dict(centres=np.asarray(sP), cbids=np.asarray(sB), B=g["B"])
    with np.errstate(over="ignore"):      # (a batch id without points has the empty box: FLT_MAX, -FLT_MAX)
        w_points = geo.window_sizes(own, r)
        w_search = w_points if g["centres"] is None else geo.window_sizes(g, r)
    cells = np.asarray(cells).astype(np.int64)
    key = np.full(len(sP), -1, np.int64)                       # the cell of every sorted point: the range that holds it
    flat = cells.reshape(-1, 2)
    for c in np.nonzero(flat[:, 1] > flat[:, 0])[0]:
        key[flat[c, 0]:flat[c, 1]] = c
    assert (key >= 0).all()
    return g, w_search, w_points, key, np.asarray(sB).reshape(-1)


def test_the_inputs_reach_every_path(oracle):
    """CPU: the paths the docstring above names, counted over the oracle's grids."""
    over256, over512 = {}, {}
    for name in geo.GEOMETRIES:
        g, w_search, w_points, key, sb = _census(oracle, name)
        over256[name] = (int((w_search > 256).sum()), int((w_points > 256).sum()))
        over512[name] = (int((w_search > 512).sum()), int((w_points > 512).sum()))
        assert len(sb) < 8192, "one member per wave"
    print("windows > 256 (search, sweeps):", over256, " > 512:", over512)
    assert min(over256["mid_windows"]) > 0 and max(over512["mid_windows"]) == 0
    assert min(over512["big_windows"]) > 0
    for name, (n, radius, scaleInv) in GROUPS.items():
        g, w_search, w_points, key, sb = _census(oracle, name)
        assert g["B"] == 2 and not sb.any(), "cloud id 1 has no points"
        for G in sorted({_group(n), min(_group(n), 4)}):   # the search and the density; its gradients
            assert G > 1 and n % (4 * G) != 0 and n % G != 0
            pad = (-n) % G
            k = np.concatenate([key, np.full(pad, -1, np.int64)]).reshape(-1, G)
            real = k >= 0
            shared = ((k[:, 1:] == k[:, :-1]) & real[:, 1:]).any(axis=1)
            spans = ((k[:, 1:] != k[:, :-1]) & real[:, 1:]).any(axis=1)
            print("%s G=%d: waves with a shared cell %d, spanning cells %d of %d" % (name, G, shared.sum(), spans.sum(), len(k)))
            assert shared.sum() > 0 and spans.sum() > 0


def _group(n):
    """Members per wave of a window kernel (csrc/batch.h: window_group)."""
    return 8 if n >= 32768 else 4 if n >= 16384 else 2 if n >= 8192 else 1
