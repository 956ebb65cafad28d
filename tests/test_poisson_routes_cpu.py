"""The designed Poisson inputs of tests/poisson_cases.py on the CPU oracle: every route and every boundary value of the dispatch
in csrc/poisson.hip is present, every planted slot decides its cell's result, and the NumPy replay of a cell's greedy walk agrees
with the oracle. This pins what tests/test_gpu_poisson_routes.py compares the kernels against. Also the census of the inputs the
suite had before (NOTES.md, "Poisson cell routes"): the assertions below keep its table true."""
import numpy as np
import pytest

from tests import poisson_cases as pc
from tests.helpers import make_cloud


@pytest.fixture(scope="module")
def pool(oracle):
    return oracle.cell_offsets_pool()


@pytest.fixture(scope="module", params=["planted", "random"])
def designed(request, oracle, pool):
    cloud = pc.design(pc.ITEMS, request.param, pool)
    return cloud, pc.reference(oracle, cloud, request.param)


def test_item_table_covers_every_route_and_boundary(designed, pool):
    cloud, ref = designed
    assert ref["cells"].shape == (len(pc.ITEMS), pc.NC, pc.NC, pc.NC, 2)
    routes, owns, totals = set(), set(), set()
    for b, it in enumerate(cloud["items"]):
        own, total, route = pc.cell_entry(ref["census"], b, it["target"])
        assert (own, total, route) == (it["own"], it["total"], it["route"]), it["name"]
        # the window's ranges hold what the design says, in table order
        assert np.array_equal(pc.window(ref["cells"][b], it["target"], pool)[1], it["counts"]), it["name"]
        routes.add(route)
        owns.add(own)
        totals.add(total)
    assert routes == set(pc.ROUTES)
    assert set(pc.OWN_EDGES) <= owns and set(pc.TOTAL_EDGES) <= totals
    by_name = {it["name"]: it for it in cloud["items"]}
    # lanes and regs and the streaming loop at the last and at the first phase; streaming with a short and a long own list
    assert {by_name[n]["phase"] for n in ("lanes2_64_128", "regs8_65_257", "stream_200_1000", "face_lanes8_60_300")} == {26}
    assert {by_name[n]["phase"] for n in ("first_lanes4_64_200", "first_regs8_65_300", "first_stream_100_800")} == {0}
    assert by_name["corner_regs4_65_200"]["phase"] == 25 and (by_name["corner_regs4_65_200"]["counts"] > 0).sum() == 8
    assert (by_name["face_lanes8_60_300"]["counts"] > 0).sum() == 18
    holes = by_name["holes_regs8_80_400"]["counts"]
    assert all(holes[o] == 0 for o in pc.HOLES) and holes[5] > 0 and holes[8] > 0 and holes[10] > 0 and holes[14] > 0
    assert any(it["route"] == "regs<2>" and 65 <= it["own"] <= 128 and it["total"] <= 128 for it in pc.ITEMS)
    assert any(it["route"] == "stream" and it["own"] <= 64 for it in pc.ITEMS)
    assert any(it["route"] == "stream" and it["own"] > 64 for it in pc.ITEMS)
    assert ref["mx"][-1, 0] - ref["mn"][-1, 0] == 2 * (ref["mx"][0, 0] - ref["mn"][0, 0])     # the box of twice the size


def test_replay_equals_the_oracle(designed, pool):
    """both kinds, every target cell: the replay reads the oracle's flags of the earlier-phase neighbours only"""
    cloud, ref = designed
    for b, it in enumerate(cloud["items"]):
        s, e = ref["cells"][(b,) + tuple(it["target"])]
        R = pc.batch_radius(ref["mn"], ref["mx"], b, cloud["radius"])
        kept = pc.replay(ref["sP"], ref["cells"][b], it["target"], R, ref["sel"], pool)
        assert np.array_equal(kept, ref["sel"][s:e]), it["name"]
    assert pc.target_kept(cloud, ref, ref["sampleIndexs"]) == [int(ref["sel"][slice(*ref["cells"][(b,) + tuple(it["target"])])].sum())
                                                               for b, it in enumerate(cloud["items"])]


def test_planted_construction_is_clean(oracle, pool):
    """Planted kind: the oracle rejects exactly the points the design says -- one per pair; every other point, the pins included,
    is selected. At a first-phase target that means: the planted own points are kept, their partners are rejected later."""
    cloud = pc.design(pc.ITEMS, "planted", pool)
    ref = pc.reference(oracle, cloud, "planted")
    assert np.array_equal(ref["sel"], ref["expected"])
    pairs = sum(len(it["plants"]) for it in cloud["items"])
    assert len(ref["sampleIndexs"]) == len(cloud["pts"]) - pairs
    assert pc.target_kept(cloud, ref, ref["sampleIndexs"]) == [it["kept"] for it in cloud["items"]]
    for b, it in enumerate(cloud["items"]):
        s, e = ref["cells"][(b,) + tuple(it["target"])]
        own_sel = ref["sel"][s:e]
        for p in it["plants"]:
            if it["first"] and p["range"] != pc.OWN:
                start, _ = pc.window(ref["cells"][b], it["target"], pool)
                assert own_sel[p["partner"]] and not ref["sel"][start[p["range"]] + p["index"]], (it["name"], p)
            else:
                assert not own_sel[p["partner"]], (it["name"], p)
        if it["first"]:
            assert it["kept"] == it["own"] - sum(1 for p in it["plants"] if p["range"] == pc.OWN)
        else:
            assert it["kept"] == it["own"] - len(it["plants"])


def test_every_planted_slot_is_decisive(oracle, pool):
    """Ignoring ONE planted slot changes the target cell's result. (A foreign slot of a first-phase target cannot decide
    anything -- no neighbour flag is set when that cell runs -- and is planted as the reverse pair, see poisson_cases.)"""
    cloud = pc.design(pc.ITEMS, "planted", pool)
    ref = pc.reference(oracle, cloud, "planted")
    for b, it in enumerate(cloud["items"]):
        s, e = ref["cells"][(b,) + tuple(it["target"])]
        R = pc.batch_radius(ref["mn"], ref["mx"], b, cloud["radius"])
        decisive = [p for p in it["plants"] if p["decisive"]]
        assert decisive, it["name"]
        for p in decisive:
            kept = pc.replay(ref["sP"], ref["cells"][b], it["target"], R, ref["sel"], pool, drop=p["slot"])
            assert not np.array_equal(kept, ref["sel"][s:e]), (it["name"], p)
            assert kept[p["partner"]] and kept.sum() == it["kept"] + 1, (it["name"], p)   # ... by exactly the pair's own point


def test_what_could_not_be_planted(pool):
    """At most one wanted slot in ten per item is left out, and never one next to a round boundary."""
    cloud = pc.design(pc.ITEMS, "planted", pool)
    for it in cloud["items"]:
        wanted, planted = it["wanted"], {p["slot"] for p in it["plants"]}
        assert set(pc.wanted_slots(it["total"])) <= set(wanted) and {0, 1, it["total"] - 2, it["total"] - 1} <= set(wanted)
        if it["starts"]:   # ... and the first slot of every non-empty range
            excl = np.cumsum(it["counts"]) - it["counts"]
            assert {int(e) for e, n in zip(excl, it["counts"]) if n} <= planted, it["name"]
        else:
            assert wanted == pc.wanted_slots(it["total"])
        assert planted | {c for c, _ in it["unplanted"]} == set(wanted)
        assert 10 * len(it["unplanted"]) <= len(wanted), (it["name"], it["unplanted"])
        assert set(pc.boundary_slots(it["total"])) <= planted, (it["name"], it["unplanted"])
        if not it["first"]:   # every slot of a last-phase target decides
            assert all(p["decisive"] for p in it["plants"])
    # the serial walk's mirrored acceptances (a pair inside the own cell) on every route
    assert {it["route"] for it in cloud["items"] if any(p["range"] == pc.OWN for p in it["plants"])} == set(pc.ROUTES)
    assert sum(len(it["unplanted"]) for it in cloud["items"]) == 0      # (as the table stands, everything wanted is planted)


def test_census_is_the_dispatch(pool):
    assert [pc.route_of(o, t) for o, t in ((1, 1), (64, 128), (65, 128), (64, 129), (65, 256), (3, 257), (70, 512), (64, 513),
                                           (65, 768), (64, 769), (65, 769), (900, 900))] == \
        ["lanes<2>", "lanes<2>", "regs<2>", "lanes<4>", "regs<4>", "lanes<8>", "regs<8>", "lanes<12>", "regs<12>", "stream",
         "stream", "stream"]
    # a 3 x 3 x 3 grid with k + 1 points in cell k: the middle cell's window is everything, a corner's is 8 cells
    n = np.arange(27) + 1
    cells = np.zeros((1, 3, 3, 3, 2), np.int32)
    cells[0, ..., 1] = np.cumsum(n).reshape(3, 3, 3)
    cells[0, ..., 0] = cells[0, ..., 1] - n.reshape(3, 3, 3)
    c = pc.census(cells)
    assert pc.cell_entry(c, 0, (1, 1, 1)) == (14, 378, "lanes<8>")
    assert pc.cell_entry(c, 0, (0, 0, 0)) == (1, 1 + 2 + 4 + 5 + 10 + 11 + 13 + 14, "lanes<2>")
    assert [pc.phase_of(3 * np.array([1, 2, 0]) + 1 + pool[p], pool) for p in range(27)] == list(range(27))


# ------------------------------------------------------------------------------------------------- the inputs the suite had
def _walk(oracle, acc, pts, bids, B, radii, scaleInv):
    """census of every level of a hierarchy over `radii` (one radius: one sampling input), added to acc"""
    mn, mx = oracle.compute_aabb(pts, bids, B, scaleInv)
    for l, r in enumerate(radii):
        k, i = oracle.sort_points_step1(pts, bids, mn, mx, B, r, scaleInv)
        sP, sB, _, cells = oracle.sort_points_step2(pts, bids, np.zeros((len(pts), 1), np.float32), k, i, mn, mx, B, r, scaleInv)
        c = pc.census(cells)
        for route, n in pc.histogram(c).items():
            acc["hist"][route] += n
        o, t = pc.edge_values(c)
        acc["own"].update(o)
        acc["total"].update(t)
        if l + 1 < len(radii):
            pts, bids, _ = oracle.poisson_sampling(sP, sB, cells, mn, mx, r, B, scaleInv)
    return acc


def _acc():
    return dict(hist={r: 0 for r in pc.ROUTES}, own=set(), total=set())


def _merge(acc, other):
    for route, n in other["hist"].items():
        acc["hist"][route] += n
    acc["own"].update(other["own"])
    acc["total"].update(other["total"])


def _reached(acc):
    return [r for r in pc.ROUTES if acc["hist"][r]]


def dense_cells_cloud():
    """the input of tests/test_gpu_parity.py::test_dense_cells"""
    rng = np.random.default_rng(13)
    blob = (0.5 + 0.012 * rng.normal(size=(900, 3))).astype(np.float32)
    rest = rng.random((400, 3), dtype=np.float32)
    pts = np.concatenate([blob, rest]).astype(np.float32)
    rng.shuffle(pts)
    return pts, np.zeros((len(pts), 1), np.int32)


def test_census_of_the_inputs_the_suite_had(oracle):
    """Which routes and boundary values the Poisson inputs of the older tests reach (the table of NOTES.md, "Poisson cell
    routes"; the counts are printed). regs<2> and a window of exactly 512 points occur nowhere, own = 64 / 65 in two hierarchy
    clouds only, regs<4> in 8 cells: tests/test_gpu_poisson_routes.py exists because of this. Not classified: levels below
    the first of the 100 000-point room (the sequential oracle needs minutes there)."""
    import math
    from mccnn_amd.workloads import modelnet_like, make_room
    from tests import ref_cases
    from tests.test_gpu_parity import CASES
    s3 = math.sqrt(3.0) + 0.1
    groups = {}
    # tests/test_gpu_parity.py: the seven CASES, test_dense_cells, test_room_absolute_radius
    a = groups["parity"] = _acc()
    one = {}
    for name, n_per, B, kind, ragged, _radius, scaleInv, _fin, prad in CASES:
        one[name] = _walk(oracle, _acc(), *make_cloud(n_per, B, 11, kind, ragged), B, [prad], scaleInv)
    one["dense_cells"] = _walk(oracle, _acc(), *dense_cells_cloud(), 1, [0.1], True)
    for c in one.values():
        _merge(a, c)
    single, dense = one["single_cell"], one["dense_cells"]
    rooms = np.concatenate([make_room(20000, 20180601), make_room(20000, 20180602)])
    _walk(oracle, a, rooms, np.repeat(np.arange(2, dtype=np.int32), 20000).reshape(-1, 1), 2, [0.2], False)
    assert dense["hist"]["stream"] == 8 and single["hist"] == dict({r: 0 for r in pc.ROUTES}, **{"regs<8>": 4})
    assert _reached(a) == ["lanes<2>", "lanes<4>", "lanes<8>", "regs<8>", "stream"]
    assert a["hist"]["regs<8>"] == 4 and a["hist"]["stream"] == 8          # ... one blob, and the four nc = 1 cells
    assert not a["own"] and a["total"] == {128, 129, 256, 257}
    # ... its other sampling tests: both forms, the fallback, the stress input
    a = groups["parity, forms / fallback / stress"] = _acc()
    for n, B, seed, kind, radius in ((4096, 1, 1, "uniform", 0.1), (3000, 3, 5, "clustered", 0.25), (600, 2, 9, "sphere", 0.6)):
        _walk(oracle, a, *make_cloud(n, B, seed, kind, True), B, [radius], True)
    _walk(oracle, a, *make_cloud(4096, 2, 3, "uniform", True), 2, [0.1], True)
    _walk(oracle, a, *modelnet_like(8192, 16, 47), 16, [0.025], True)
    assert _reached(a) == ["lanes<2>", "lanes<4>", "lanes<8>", "lanes<12>", "regs<8>", "regs<12>", "stream"]
    assert not a["own"] and a["total"] == {769}
    # tests/test_gpu_hierarchy.py, every level
    a = groups["hierarchy"] = _acc()
    _walk(oracle, a, *make_cloud(3000, 5, 3, "clustered", True), 5, [0.1, 0.4, s3], True)
    _walk(oracle, a, *make_cloud(3000, 4, 5, "clustered", True), 4, [0.1, 0.4], True)
    _walk(oracle, a, *make_cloud(2500, 4, 9, "clustered", True), 4, [0.1, 0.3, 0.9], True)
    room = make_room(100000, 20180601)
    _walk(oracle, a, room, np.zeros((len(room), 1), np.int32), 1, [0.1], False)          # (first level only)
    assert _reached(a) == ["lanes<2>", "lanes<4>", "lanes<8>", "lanes<12>", "regs<4>", "regs<8>", "regs<12>"]
    assert a["own"] == {64, 65} and a["total"] == {128, 129, 256, 257}
    # tests/test_gpu_configs.py: cfg1 .. cfg3, every level
    a = groups["configs"] = _acc()
    _walk(oracle, a, *modelnet_like(1024, 32, 41), 32, [0.1, 0.4, s3], True)
    _walk(oracle, a, *modelnet_like(4096, 32, 43), 32, [0.1, 0.4, s3], True)
    _walk(oracle, a, *modelnet_like(8192, 16, 47), 16, [0.025, 0.1, 0.4], True)
    assert _reached(a) == ["lanes<2>", "lanes<4>", "lanes<8>", "lanes<12>"]
    assert not a["own"] and a["total"] == {128, 129, 256, 257, 513}
    # tests/ref_cases.py
    a = groups["ref_cases"] = _acc()
    for case in ref_cases.CASES:
        inp = ref_cases.make_inputs(case) if case["prads"] else None
        for prad in case["prads"]:
            _walk(oracle, a, inp["pts"], inp["bids"], case["B"], [prad], case["scaleInv"])
    assert _reached(a) == ["lanes<2>", "lanes<4>", "lanes<8>", "lanes<12>", "regs<8>", "stream"]
    assert not a["own"] and a["total"] == {128, 129, 257, 768}
    for name, a in groups.items():
        print("%-36s %s own %s total %s" % (name, {r: n for r, n in a["hist"].items() if n}, sorted(a["own"]), sorted(a["total"])))
    assert all(a["hist"]["regs<2>"] == 0 and 512 not in a["total"] for a in groups.values())
