"""TEST INFRASTRUCTURE shared by tests/test_poisson_routes_cpu.py and tests/test_gpu_poisson_routes.py: the cell routes of
csrc/poisson.hip, a census that names the route of every occupied cell of a cell table, a designer of clouds whose target
cells have an exact (own, total), and the NumPy replay of one cell's greedy walk.

THE ROUTES. poisson_cell runs one wave per occupied cell. With own = the cell's points and total = the points of its 27-cell
window (MCCNN_PS_ROUNDS = 12 rounds of 64 register slots):
  total > 768               the streaming loop
  total <= 768, own <= 64   poisson_cell_lanes<NR>
  total <= 768, own >  64   poisson_cell_regs<NR>          NR = 2, 4, 8, 12 from ceil(total / 64)
The window is one flat list of `total` slots: the 27 ranges in the order of the pool table (oracle.cell_offsets_pool(), the
cell's own range is entry 17), each range in the cell's sorted order. Slot c lives in lane c & 63 of round c >> 6.

THE DESIGNED CLOUDS. One batch item per entry of ITEMS: a target cell of a 10^3 grid, its own count, its window total, and how
total - own is spread over the neighbours. Two pin points per item, at the box corners, make the box 10 cells wide. The input
goes cell by cell; the sort is stable inside a cell, so the in-cell order -- and with it the flat slot order -- is the
designer's. Two kinds:
  random   points uniform inside their cells, radius = cell size: the product's use. About one point per cell survives and
           2 to 7 of the window's slots decide the result, so this kind checks route coverage, not every slot.
  planted  the grid is built at cell size h, the sampling runs with r = h / 50 (the op takes the radius apart from the cell
           table). Points sit on a jittered 8 x 8 x 8 sub-lattice of their cell (pitch h / 8, jitter 0.02 h: every two points
           are >= 0.085 h = 4.25 r apart, every point >= 0.0425 h from the faces of its cell), so every point is selected --
           except where a PAIR is planted: for a wanted slot in a neighbour of an earlier phase that point is moved to
           0.004 h = 0.2 r beyond the shared face / edge / corner and one own point of the target to the mirrored place
           (distance 0.008 h, 0.0113 h, 0.0139 h < r = 0.02 h); that own point is rejected if and only if the kernel reads the
           flag and the coordinates of exactly that slot. Tangential places of a face (15 x 15) and of an edge (15) are 0.05 h
           apart and >= 0.15 h from the cell's other faces, so planted pairs do not see each other. A wanted slot in the own
           cell keeps its place and a LATER own point is moved to 0.008 h beside it: the later one is rejected through the
           mirrored acceptance of the serial walk. Wanted are slots 0, 1, total - 2, total - 1 and 64 k - 2 .. 64 k + 1 for every
           64 k < total; items with `starts` add the first slot of every non-empty range of the window.
           A target of the FIRST phase runs before all its neighbours: no neighbour flag is set, a foreign slot cannot decide
           anything there. The pair is planted all the same (`decisive` False): the own point must be KEPT (a kernel that
           takes an unselected candidate for a selected one rejects it) and the neighbour's point is rejected later, when the
           neighbour's window reads the target's flags.
What cannot be planted: a corner neighbour shares one point with the target (one pair), the pin points do not move, the last
own point has no later own point, and every pair needs an own point of its own -- `unplanted` lists slot and reason.
"""
import numpy as np

NC = 10                   # cells per axis
CELL = 0.1                # cell size handed to the sort ops (scaleInv: relative to the box) -> 10 cells
BOX = 1.25                # box extent: BOX / NC = 0.125 exactly, in float32 as well
ROUNDS, LANES = 12, 64    # MCCNN_PS_ROUNDS, the wave
OWN = 17                  # the cell's own range in the pool table: offset (0, 0, 0)
PLANT_RADIUS = CELL / 50  # planted kind: r = h / 50
ROUTES = ["lanes<2>", "lanes<4>", "lanes<8>", "lanes<12>", "regs<2>", "regs<4>", "regs<8>", "regs<12>", "stream"]
OWN_EDGES = (64, 65)
TOTAL_EDGES = (128, 129, 256, 257, 512, 513, 768, 769)

DELTA = 0.004             # a planted point's distance from the shared face, in cells (0.2 r)
BESIDE = 0.008            # own-own pair: the later point's distance from the earlier one, in cells (0.4 r)
JITTER = 0.02             # sub-lattice jitter, in cells


# ------------------------------------------------------------------------------------------------- census
def route_of(own, total):
    """the dispatch of poisson_cell (csrc/poisson.hip)"""
    if total > LANES * ROUNDS:
        return "stream"
    nr = (total + LANES - 1) // LANES
    return "%s<%d>" % ("lanes" if own <= LANES else "regs", 2 if nr <= 2 else 4 if nr <= 4 else 8 if nr <= 8 else ROUNDS)


def census(cells):
    """cell table [B, nc, nc, nc, 2] -> per OCCUPIED cell: b, x, y, z, own, total (its 27-window), route. NumPy, from the table
    alone."""
    cells = np.asarray(cells)
    own = (cells[..., 1] - cells[..., 0]).astype(np.int64)
    nc = own.shape[1]
    pad = np.pad(own, ((0, 0), (1, 1), (1, 1), (1, 1)))
    total = np.zeros_like(own)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                total += pad[:, dx:dx + nc, dy:dy + nc, dz:dz + nc]
    b, x, y, z = np.nonzero(own > 0)
    o, t = own[b, x, y, z], total[b, x, y, z]
    return dict(b=b, x=x, y=y, z=z, own=o, total=t, route=np.array([route_of(int(a), int(c)) for a, c in zip(o, t)], dtype=object))


def histogram(c):
    """census -> {route: cells}, every route named"""
    return {r: int((c["route"] == r).sum()) for r in ROUTES}


def edge_values(c):
    """census -> which of the boundary values of own and total occur among the occupied cells"""
    return sorted(set(c["own"].tolist()) & set(OWN_EDGES)), sorted(set(c["total"].tolist()) & set(TOTAL_EDGES))


def cell_entry(c, b, cell):
    """(own, total, route) of one cell of a census"""
    m = np.nonzero((c["b"] == b) & (c["x"] == cell[0]) & (c["y"] == cell[1]) & (c["z"] == cell[2]))[0]
    if len(m) == 0:
        return 0, 0, None
    return int(c["own"][m[0]]), int(c["total"][m[0]]), c["route"][m[0]]


# ------------------------------------------------------------------------------------------------- phases and windows
def phase_of(cell, pool):
    """colour phase of a cell: cell = 3 g + 1 + pool[phase] (pool = oracle.cell_offsets_pool())"""
    off = np.array([int(c) % 3 - 1 for c in cell])
    return int(np.nonzero((np.asarray(pool) == off).all(axis=1))[0][0])


def window(cells_b, cell, pool):
    """the 27 ranges of a cell's window in table order -> (start[27], count[27]); a range outside the grid is empty"""
    nc = cells_b.shape[0]
    start, count = np.zeros(27, np.int64), np.zeros(27, np.int64)
    for o in range(27):
        q = [int(cell[a]) + int(pool[o][a]) for a in range(3)]
        if all(0 <= v < nc for v in q):
            s, e = cells_b[q[0], q[1], q[2]]
            start[o], count[o] = s, e - s
    return start, count


def slot_range(count, c):
    """flat slot c -> (range, index inside the range): the largest range whose exclusive offset is <= c and that is not empty"""
    incl = np.cumsum(count)
    o = int(np.searchsorted(incl, c, side="right"))
    return o, int(c - (incl[o] - count[o]))


def wanted_slots(total):
    """0, 1, total - 2, total - 1 and 64 k - 2 .. 64 k + 1 for every 64 k < total"""
    w = {0, 1, total - 2, total - 1}
    for k in range(1, (total - 1) // LANES + 1):
        w.update(range(LANES * k - 2, LANES * k + 2))
    return sorted(c for c in w if 0 <= c < total)


def boundary_slots(total):
    """both slots next to every round boundary: 64 k - 1 and 64 k"""
    return sorted(c for k in range(1, (total - 1) // LANES + 1) for c in (LANES * k - 1, LANES * k) if c < total)


# ------------------------------------------------------------------------------------------------- the item table
LAST, FIRST = (3, 3, 5), (5, 5, 3)        # interior cells of phase 26 (every neighbour earlier) and of phase 0 (every one later)
HOLES = (6, 7, 11, 12, 13)                # spread "holes": these entries of the table stay empty -- equal offsets in the search


def _item(name, target, own, total, spread="default", scale=1.0, starts=False):
    """starts: the first slot of every non-empty range is wanted too -- the slot search (`largest s with excl_s <= c`) at every
    range boundary, behind empty ranges included"""
    return dict(name=name, target=target, own=own, total=total, spread=spread, scale=scale, starts=starts,
                route=route_of(own, total))


ITEMS = [
    _item("lanes2_64_128", LAST, 64, 128),
    _item("regs2_65_128", LAST, 65, 128),
    _item("regs2_100_120", LAST, 100, 120),
    _item("lanes4_64_129", LAST, 64, 129),
    _item("regs4_65_129", LAST, 65, 129),
    _item("lanes4_40_256", LAST, 40, 256),
    _item("regs4_70_256", LAST, 70, 256),
    _item("lanes8_64_257", LAST, 64, 257, starts=True),
    _item("regs8_65_257", LAST, 65, 257),
    _item("lanes8_48_512", LAST, 48, 512),
    _item("regs8_130_512", LAST, 130, 512),
    _item("lanes12_50_513", LAST, 50, 513),
    _item("regs12_90_513", LAST, 90, 513),
    _item("lanes12_64_768", LAST, 64, 768),
    _item("regs12_65_768", LAST, 65, 768),
    _item("stream_64_769", LAST, 64, 769),
    _item("stream_65_769", LAST, 65, 769),
    _item("stream_200_1000", LAST, 200, 1000, starts=True),
    _item("corner_regs4_65_200", (0, 0, 0), 65, 200, starts=True),    # grid corner (phase 25): 19 ranges outside the grid, own holds a pin
    _item("face_lanes8_60_300", (0, 3, 5), 60, 300, starts=True),    # grid face (phase 26): 9 ranges outside the grid
    _item("holes_regs8_80_400", LAST, 80, 400, "holes", starts=True),    # empty neighbours in the middle of the table order
    _item("first_lanes4_64_200", FIRST, 64, 200),
    _item("first_regs8_65_300", FIRST, 65, 300, starts=True),
    _item("first_stream_100_800", FIRST, 100, 800),
    _item("box2_regs8_65_257", LAST, 65, 257, scale=2.0),   # a box twice the size: R and the threshold are per batch item
]
SMALL_ITEMS = [ITEMS[1], ITEMS[3]]   # the small cloud of the workspace-reuse test


def neighbour_counts(item, pool):
    """points per range of the target's window, table order: the corner neighbours hold one point each (one planted pair is
    all a corner can carry), the rest goes evenly over the face and edge neighbours inside the grid"""
    t = item["target"]
    inside = [o for o in range(27) if all(0 <= t[a] + int(pool[o][a]) < NC for a in range(3))]
    if item["spread"] == "holes":
        inside = [o for o in inside if o not in HOLES]
    nz = {o: int(np.count_nonzero(pool[o])) for o in inside}
    count = np.zeros(27, np.int64)
    count[OWN] = item["own"]
    rest = item["total"] - item["own"]
    for o in inside:
        if nz[o] == 3 and rest > 0:
            count[o] = 1
            rest -= 1
    wide = [o for o in inside if nz[o] in (1, 2)]
    for n, o in enumerate(wide):
        count[o] = rest // len(wide) + (1 if n < rest % len(wide) else 0)
    # a wanted slot among the last own points finds no later own point to pair with: move the own range up the window, twelve
    # points at a time from the neighbours behind it in the table to those in front of it
    before, behind = [o for o in wide if o < OWN], [o for o in wide if o > OWN]
    for _ in range(4):
        end = int(count[:OWN + 1].sum())
        if not any(end - 8 <= c < end for c in wanted_slots(item["total"])) or not before:
            break
        for _ in range(12):
            give = max(behind, key=lambda o: count[o], default=None)
            if give is None or count[give] == 0:
                break
            count[give] -= 1
            count[min(before, key=lambda o: count[o])] += 1
    assert count.sum() == item["total"] and count.max() <= 400, item["name"]
    return count


# ------------------------------------------------------------------------------------------------- the designer
def _lattice(rng, n):
    """n points of one cell on the jittered 8^3 sub-lattice, in cells, random order"""
    site = rng.permutation(512)[:n]
    ijk = np.stack([site // 64, (site // 8) % 8, site % 8], axis=1)
    return (ijk + 0.5) / 8.0 + JITTER * (2.0 * rng.random((n, 3)) - 1.0)


def design(items, kind, pool, seed=5):
    """-> cloud: pts [N, 3] f32, bids [N, 1] i32, B, cell (the sort's cell size), radius (the sampling's), kind, and per batch item
    `items[b]`: the entry of the table plus counts[27], phase, first (a first-phase target), wanted, plants, unplanted,
    rejected (input indices of the points the design expects to be rejected), kept (expected samples of the target cell)."""
    assert kind in ("random", "planted")
    rng = np.random.default_rng(seed)
    pool = np.asarray(pool)
    pts, bids, out = [], [], []
    base = 0
    for b, it in enumerate(items):
        it = dict(it)
        t = np.array(it["target"])
        count = neighbour_counts(it, pool)
        ph = phase_of(t, pool)
        nph = [phase_of(t + pool[o], pool) for o in range(27) if o != OWN and count[o] > 0]
        assert all(p < ph for p in nph) or all(p > ph for p in nph), it["name"]
        it.update(counts=count, phase=ph, first=bool(nph) and nph[0] > ph, plants=[], unplanted=[], wanted=[])
        # points per range, in cells; the pin of cell (0, 0, 0) is the first point of that cell
        local = []
        for o in range(27):
            n = int(count[o])
            p = _lattice(rng, n) if kind == "planted" else 0.001 + 0.998 * rng.random((n, 3))
            local.append(p + (t + pool[o]))
        pin_own = tuple(it["target"]) == (0, 0, 0)
        if pin_own:
            local[OWN][0] = 0.0
        assert tuple(it["target"]) != (NC - 1,) * 3
        first_idx = np.concatenate([[0], np.cumsum(count)])[:27]     # input index of a range's first point, inside the item
        rejected = []
        if kind == "planted":
            starts = (np.cumsum(count) - count)[count > 0].tolist() if it["starts"] else []
            it["wanted"] = sorted(set(wanted_slots(it["total"])) | set(starts))
            rejected = _plant(it, local, pool, pin_own)
        block = np.concatenate(local + [np.zeros((0 if pin_own else 1, 3)), np.full((1, 3), float(NC))])
        it["input"] = base + first_idx                                # ... in the whole cloud
        it["rejected"] = [base + int(first_idx[o]) + int(i) for o, i in rejected]
        it["kept"] = it["own"] - sum(1 for o, _ in rejected if o == OWN) if kind == "planted" else None
        pts.append(block * (BOX / NC * it["scale"]))
        bids.append(np.full((len(block), 1), b, np.int32))
        base += len(block)
        out.append(it)
    return dict(pts=np.concatenate(pts).astype(np.float32), bids=np.concatenate(bids), B=len(items), cell=CELL,
                radius=CELL if kind == "random" else PLANT_RADIUS, kind=kind, items=out)


def _plant(it, local, pool, pin_own):
    """moves points of `local` so that the wanted slots decide; -> [(range, index)] of the points that must be rejected"""
    t, count = np.array(it["target"]), it["counts"]
    where = {c: slot_range(count, c) for c in it["wanted"]}
    own_wanted = {i for o, i in where.values() if o == OWN}
    free = [i for i in range(it["own"]) if i not in own_wanted and not (pin_own and i == 0)]   # own points a pair may move
    places = {}       # neighbour range -> tangential places handed out
    rejected = []

    def fail(c, why):
        it["unplanted"].append((c, why))

    # own slots first: their partners have to come LATER in the cell, the foreign pairs take any own point
    for c in reversed(it["wanted"]):   # the last one first: it has the fewest later points to choose from
        o, i = where[c]
        if o != OWN:
            continue
        later = [j for j in free if j > i]
        if not later:
            fail(c, "no later own point")
            continue
        j = later[-1]
        free.remove(j)
        a = local[OWN][i]
        step = np.array([BESIDE if a[0] - t[0] < 0.5 else -BESIDE, 0.0, 0.0])    # towards the middle of the cell
        local[OWN][j] = a + step
        rejected.append((OWN, j))
        it["plants"].append(dict(slot=c, range=OWN, index=i, partner=j, decisive=True))
    for c in it["wanted"]:
        o, i = where[c]
        if o == OWN:
            continue
        d = pool[o]
        nz = int(np.count_nonzero(d))
        n = places.get(o, 0)
        if n >= (225, 15, 1)[nz - 1]:
            fail(c, "corner neighbour: one pair" if nz == 3 else "no place left on the face / edge")
            continue
        if not free:
            fail(c, "no own point left")
            continue
        places[o] = n + 1
        j = free.pop(0)
        tang = [0.15 + 0.05 * (n % 15), 0.15 + 0.05 * (n // 15)]
        there, here = np.zeros(3), np.zeros(3)
        for a in range(3):
            if d[a] == 0:
                there[a] = here[a] = t[a] + tang.pop(0)
            else:
                plane = t[a] + (1 if d[a] > 0 else 0)
                there[a], here[a] = plane + d[a] * DELTA, plane - d[a] * DELTA
        local[o][i], local[OWN][j] = there, here
        # last-phase target: the neighbour's point is selected first and rejects the own point; first-phase target: the own
        # point is selected first and rejects the neighbour's point when that cell runs
        rejected.append((o, i) if it["first"] else (OWN, j))
        it["plants"].append(dict(slot=c, range=o, index=i, partner=j, decisive=not it["first"]))
    return rejected


# ------------------------------------------------------------------------------------------------- reference and replay
_REFERENCE = {}


def reference(oracle, cloud, key=None):
    """the oracle's chain on a designed cloud, computed once per key: boxes, both sort steps, the sampling, its selection mask
    over the sorted points, the census, and the expected mask of a planted cloud"""
    if key is not None and key in _REFERENCE:
        return _REFERENCE[key]
    pts, bids, B = cloud["pts"], cloud["bids"], cloud["B"]
    mn, mx = oracle.compute_aabb(pts, bids, B, True)
    keys, idx = oracle.sort_points_step1(pts, bids, mn, mx, B, cloud["cell"], True)
    feats = np.zeros((len(pts), 1), np.float32)
    sP, sB, _, cells = oracle.sort_points_step2(pts, bids, feats, keys, idx, mn, mx, B, cloud["cell"], True)
    sp, sb, si = oracle.poisson_sampling(sP, sB, cells, mn, mx, cloud["radius"], B, True)
    sel = np.zeros(len(pts), bool)
    sel[si] = True
    r = dict(mn=mn, mx=mx, keys=keys, idx=idx, sP=sP, sB=sB, cells=cells, samplePts=sp, sampleBatchs=sb, sampleIndexs=si,
             transformedIndexs=oracle.transform_indexs(si, idx), sel=sel, census=census(cells))
    if cloud["kind"] == "planted":
        exp = np.ones(len(pts), bool)
        for it in cloud["items"]:
            exp[idx[np.array(it["rejected"], np.int64)]] = False
        r["expected"] = exp
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    if key is not None:
        _REFERENCE[key] = r
    return r


def batch_radius(mn, mx, b, radius):
    """R of one batch item (scaleInv): radius * max extent, in float32 like the kernels"""
    return np.float32(radius) * np.float32((np.asarray(mx, np.float32)[b] - np.asarray(mn, np.float32)[b]).max())


def replay(sP, cells_b, target, R, flags, pool, drop=None):
    """The greedy walk of ONE cell (poisson_sampling.cu:51-124) in NumPy: sP the sorted points, cells_b the batch item's cell
    table, R its radius, flags the selection of the whole cloud -- only the flags of the window's EARLIER-phase cells are read,
    the cell's own ones are computed here. drop: this flat slot of the window is ignored as a candidate.
    -> bool[own]: which of the cell's points are kept."""
    start, count = window(cells_b, target, pool)
    ph = phase_of(target, pool)
    j = np.concatenate([np.arange(start[o], start[o] + count[o]) for o in range(27)]).astype(np.int64)
    rng = np.repeat(np.arange(27), count)
    earlier = np.array([phase_of(np.array(target) + pool[o], pool) < ph if count[o] else False for o in range(27)])
    sel = np.asarray(flags, bool)[j] & earlier[rng]
    heard = np.ones(len(j), bool)
    if drop is not None:
        heard[drop] = False
    own0 = int(np.cumsum(count)[OWN] - count[OWN])
    q = np.asarray(sP, np.float32)[j]
    R = np.float32(R)
    kept = np.zeros(int(count[OWN]), bool)
    for i in range(int(count[OWN])):
        d = q - q[own0 + i]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
        if not np.any(sel & heard & (dist < R)):
            kept[i] = sel[own0 + i] = True
    return kept


def target_kept(cloud, ref, sample_indexs):
    """per batch item: how many of the given sample indices lie in the target cell"""
    si = np.asarray(sample_indexs)
    out = []
    for b, it in enumerate(cloud["items"]):
        s, e = ref["cells"][(b,) + tuple(it["target"])]
        out.append(int(((si >= s) & (si < e)).sum()))
    return out


def describe_mismatch(cloud, ref, got_indexs):
    """'' when the sample indices equal the oracle's; otherwise the first differing batch item with its (own, total, route) and
    the cell of the first differing point with its own census entry -- the route is then known without another run"""
    got, want = np.asarray(got_indexs).reshape(-1), ref["sampleIndexs"]
    if got.shape == want.shape and np.array_equal(got, want):
        return ""
    n = len(ref["sel"])
    if got.size and (got.min() < 0 or got.max() >= n):
        return "sample indices outside [0, %d)" % n
    sel = np.zeros(n, bool)
    sel[got] = True
    diff = np.nonzero(sel != ref["sel"])[0]
    if len(diff) == 0:
        return "the same %d samples in another order (or repeated)" % len(want)
    p = int(diff[0])
    b = int(ref["sB"][p, 0])
    it = cloud["items"][b]
    cb = ref["cells"][b]
    x, y, z = [int(v[0]) for v in np.nonzero((cb[..., 0] <= p) & (p < cb[..., 1]))]
    own, total, route = cell_entry(ref["census"], b, (x, y, z))
    return ("%d points differ; first: sorted point %d (%s by the oracle) of batch item %d = %s, target %s (own %d, total %d, %s); "
            "the point's cell (%d, %d, %d) has own %d, total %d, %s; %d differing points in this item"
            % (len(diff), p, "kept" if ref["sel"][p] else "rejected", b, it["name"], tuple(it["target"]), it["own"], it["total"],
               it["route"], x, y, z, own, total, route, int((ref["sB"][diff, 0] == b).sum())))
