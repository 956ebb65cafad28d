"""Every cell route of csrc/poisson.hip and every window-slot boundary, on the designed clouds of tests/poisson_cases.py (pinned
on the CPU by tests/test_poisson_routes_cpu.py): ~25 batch items of one cloud, ~10 k points, 10^3 cells per item; each item's
target cell has an exact (own, total) and so takes one known route. The planted kind makes the slots next to every round
boundary (64 k - 2 .. 64 k + 1), the first two and the last two decide the cell's result; the random kind is the product's use
(radius = cell size). Both go through mc.poisson_sampling in its three call forms; the random kind also through the fused
hierarchy level. Everything compared is integers or copied floats: exact, in the oracle's order."""
import numpy as np
import pytest

from tests import poisson_cases as pc

pytestmark = pytest.mark.gpu

FORMS = [(False, "phased"), (True, "dataflow"), (2, "nospin_fallback")]


def _wrap(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def pool(oracle):
    return oracle.cell_offsets_pool()


def _designed(oracle, pool, kind, items=None):
    cloud = pc.design(pc.ITEMS if items is None else items, kind, pool)
    return cloud, pc.reference(oracle, cloud, kind if items is None else None)


def _grid(mc, cloud, ref):
    """boxes and both sort steps on the GPU, compared exactly with the oracle's"""
    import torch
    B = cloud["B"]
    P, Bi = _wrap(cloud["pts"]), _wrap(cloud["bids"])
    mn, mx = mc.compute_aabb(P, Bi, B, True)
    keys, idx = mc.sort_points_step1(P, Bi, mn, mx, B, cloud["cell"], True)
    feats = torch.zeros((len(cloud["pts"]), 1), device="cuda")
    sP, sB, _, cells = mc.sort_points_step2(P, Bi, feats, keys, idx, mn, mx, B, cloud["cell"], True)
    g = dict(P=P, Bi=Bi, mn=mn, mx=mx, keys=keys, idx=idx, sP=sP, sB=sB, cells=cells)
    for k in ("mn", "mx", "keys", "idx", "sP", "sB", "cells"):
        got = _unwrap(g[k])
        assert got.shape == ref[k].shape and np.array_equal(got, ref[k]), k
    return g


def _sample(mc, cloud, ref, g, what):
    """one mc.poisson_sampling call against the oracle; a mismatch names the first differing item and its route"""
    sp, sb, si = mc.poisson_sampling(g["sP"], g["sB"], g["cells"], g["mn"], g["mx"], cloud["radius"], cloud["B"], True)
    si_h = _unwrap(si)
    msg = pc.describe_mismatch(cloud, ref, si_h)
    assert not msg, "%s: %s" % (what, msg)
    assert np.array_equal(_unwrap(sp), ref["samplePts"]) and np.array_equal(_unwrap(sb), ref["sampleBatchs"]), what
    want = [it["kept"] for it in cloud["items"]] if cloud["kind"] == "planted" else pc.target_kept(cloud, ref, ref["sampleIndexs"])
    got = pc.target_kept(cloud, ref, si_h)
    assert got == want, (what, [(it["name"], a, b) for it, a, b in zip(cloud["items"], got, want) if a != b])
    return sp, sb, si


@pytest.mark.parametrize("form", FORMS, ids=[f[1] for f in FORMS])
@pytest.mark.parametrize("kind", ["planted", "random"])
def test_every_route_in_every_call_form(mc, oracle, pool, kind, form):
    """phased (one launch per colour phase), dataflow (one launch, cells wait on flags) and the dataflow form without spinning,
    which gives up at the first unfinished neighbour and repeats phased (the project's POISSON_DATAFLOW = 2 switch). One batch
    item (box2_*) has a box of twice the size: R and the threshold are per batch item, the planted distances scale with it."""
    flag, name = form
    cloud, ref = _designed(oracle, pool, kind)
    assert set(it["route"] for it in cloud["items"]) == set(pc.ROUTES)
    g = _grid(mc, cloud, ref)
    before = mc.POISSON_FALLBACKS
    mc.POISSON_DATAFLOW = flag
    try:
        _sample(mc, cloud, ref, g, "%s, %s" % (kind, name))
    finally:
        mc.POISSON_DATAFLOW = True
    if flag is True:
        assert mc.POISSON_FALLBACKS == before
    elif flag == 2:
        assert mc.POISSON_FALLBACKS == before + 1


@pytest.mark.parametrize("form", FORMS[:2], ids=[f[1] for f in FORMS[:2]])
def test_workspace_reuse_large_small_large(mc, oracle, pool, form):
    """The library's scratch buffer only grows: the small cloud's call finds the large one's selection bytes, slot counters,
    done flags and cell lists in it, the large one's second call those of the small one. Each call clears what it reads."""
    flag, name = form
    large, ref_l = _designed(oracle, pool, "planted")
    small, ref_s = _designed(oracle, pool, "planted", pc.SMALL_ITEMS)
    assert len(small["pts"]) < len(large["pts"]) // 10
    g_l, g_s = _grid(mc, large, ref_l), _grid(mc, small, ref_s)
    mc.POISSON_DATAFLOW = flag
    try:
        for rep, (cloud, ref, g) in enumerate(((large, ref_l, g_l), (small, ref_s, g_s), (large, ref_l, g_l))):
            _sample(mc, cloud, ref, g, "%s, call %d" % (name, rep))
    finally:
        mc.POISSON_DATAFLOW = True


def test_fused_hierarchy_level_reaches_every_route(mc, oracle, pool):
    """mc.point_hierarchy_levels (mccnn_hierarchy_level: grid, sampling and index transform in one call, the sampling in its
    dataflow form) on the random kind: level 0 equals the op-by-op chain and the oracle. The fused level builds its grid AT the
    radius, so the planted kind (radius = cell / 50) cannot go through it: this checks the route coverage of that entry only,
    the slot boundaries are checked through mc.poisson_sampling above."""
    cloud, ref = _designed(oracle, pool, "random")
    g = _grid(mc, cloud, ref)
    assert mc.POISSON_DATAFLOW is True
    before = mc.POISSON_FALLBACKS
    sp, sb, si = _sample(mc, cloud, ref, g, "op by op")
    ti = mc.transform_indexs(si, g["idx"])
    lv = mc.point_hierarchy_levels(g["P"], g["Bi"], g["mn"], g["mx"], [cloud["cell"]], cloud["B"], True)
    assert lv is not None and len(lv) == 1 and mc.POISSON_FALLBACKS == before
    fp, fb, fi, ft = [_unwrap(t) for t in lv[0]]
    msg = pc.describe_mismatch(cloud, ref, fi)
    assert not msg, "fused level: " + msg
    for got, chain, want in ((fp, sp, ref["samplePts"]), (fb, sb, ref["sampleBatchs"]), (fi, si, ref["sampleIndexs"]),
                             (ft, ti, ref["transformedIndexs"])):
        assert got.shape == want.shape and np.array_equal(got, want) and np.array_equal(got, _unwrap(chain))
