"""NumPy float32 restatement of the device batcher's kernel (mccnn_amd/csrc/batch_sample.hip): the same plan (the slot
records of mccnn_amd.device_batcher.SLOT_DTYPE) over the same store gives the source rows, batch ids, rotated points,
counts and status words the kernel writes. Every f32 expression is spelled in the kernel's operand order with np.float32
operands (no Python float ever meets an np.float32 scalar: that would promote to double on older NumPy)."""
import numpy as np

F = np.float32
U32 = np.uint64(0xFFFFFFFF)
MAX_PASSES = 64
OK, NO_POINT, PASS_BOUND = 0, 1, 2
SCREEN = 128


def mix(x):
    """murmur3 finaliser on uint32 values (held in uint64 so that NumPy never warns about the wrap)."""
    x = np.asarray(x, np.uint64) & U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & U32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & U32
    x ^= x >> np.uint64(16)
    return x


def pass_hash(seed, t):
    return mix((np.uint64(int(seed)) + np.uint64(0x9E3779B9) * np.uint64(t + 1)) & U32)


def draws(seed, t, n):
    """u of pass t for the points 0 .. n-1 of a model: exact multiples of 2^-24 in [0, 1)."""
    d = mix((pass_hash(seed, t) + np.arange(n, dtype=np.uint64)) & U32) >> np.uint64(8)
    return d.astype(F) * F(2.0 ** -24)


def uniform_indices(n, K, seed):
    """The uniform protocol: K rows over the first n points."""
    a = pass_hash(seed, 0)
    t = np.arange(K, dtype=np.uint64)
    h = mix((a + t) & U32)
    if n < K:
        return ((h * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    lo = t * np.uint64(n) // np.uint64(K)
    hi = (t + np.uint64(1)) * np.uint64(n) // np.uint64(K)
    return (lo + ((h * (hi - lo)) >> np.uint64(32))).astype(np.int64)


def _axis(slot):
    size = slot["bmax"].astype(F) - slot["bmin"].astype(F)
    ax, s = 0, size[0]
    if size[1] > s:
        ax, s = 1, size[1]
    if size[2] > s:
        ax, s = 2, size[2]
    return ax, s, F(slot["bmin"][ax])


def probabilities(slot, pts, normals):
    """f32 acceptance probabilities of protocols 1 (split), 2 (gradient), 3 (lambert) for the model's points."""
    proto = int(slot["protocol"])
    pts = np.asarray(pts, F)
    with np.errstate(all="ignore"):
        if proto == 3:
            v = slot["view"].astype(F)
            nr = np.asarray(normals, F)
            d = nr[:, 0] * v[0] + nr[:, 1] * v[1] + nr[:, 2] * v[2]
            c = np.where(d > F(0), d, F(0)).astype(F)
            c = np.where(c < F(1), c, F(1)).astype(F)
            return np.sqrt(c)
        ax, size, lo = _axis(slot)
        x = pts[:, ax]
        if proto == 1:
            pos = (x - lo) / size
            return np.where(pos > F(0.5), F(1.0), F(0.25)).astype(F)
        p = (x - lo - size * F(0.2)) / (size * F(0.6))
        c = np.where(p > F(0.01), p, F(0.01)).astype(F)
        c = np.where(c < F(1), c, F(1)).astype(F)
        return np.sqrt(c)


def _pixel(t, pixel):
    q = np.floor(t / pixel)
    q = np.where(q >= F(-1073741824.0), q, F(-1073741824.0))
    q = np.where(q <= F(1073741824.0), q, F(1073741824.0))
    return q.astype(np.int64) & (SCREEN - 1)


def occlusion_keep(slot, pts, normals):
    """Keep mask of protocol 4 for the model's points."""
    pts, nr = np.asarray(pts, F), np.asarray(normals, F)
    with np.errstate(all="ignore"):
        vx, vy, vz = (F(c) for c in slot["view"])
        ax, az = -vz, vx
        xl = np.sqrt(ax * ax + az * az)
        xx, xy, xz = ax / xl, F(0), az / xl
        bx, by, bz = -(xz * vy), xz * vx - xx * vz, xx * vy
        yl = np.sqrt(bx * bx + by * by + bz * bz)
        yx, yy, yz = bx / yl, by / yl, bz / yl
        mn, mx = slot["bmin"].astype(F), slot["bmax"].astype(F)
        d = mx - mn
        diag = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) * F(0.5)
        c = (mx + mn) * F(0.5)
        pixel = diag / F(SCREEN // 2)
        depth = diag * F(2.0)
        sx = c[0] - vx * diag - xx * diag - yx * diag
        sy = c[1] - vy * diag - xy * diag - yy * diag
        sz = c[2] - vz * diag - xz * diag - yz * diag
        t0, t1, t2 = pts[:, 0] - sx, pts[:, 1] - sy, pts[:, 2] - sz
        tx = t0 * xx + t1 * xy + t2 * xz
        ty = t0 * yx + t1 * yy + t2 * yz
        z = ((t0 * vx + t1 * vy + t2 * vz) / depth).astype(F)
        pix = _pixel(tx, pixel) * SCREEN + _pixel(ty, pixel)
        facing = (nr[:, 0] * vx + nr[:, 1] * vy + nr[:, 2] * vz) < F(0)
        bits = z.view(np.uint32)
        key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
        zb = np.full(SCREEN * SCREEN, 0xFFFFFFFF, np.uint32)
        np.minimum.at(zb, pix[facing], key[facing])
        k = zb[pix]
        zmin = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(F)
        return facing & ((z - zmin) < F(0.01))


def select(slot, pts, normals):
    """-> (model-local indices of the rows the slot produces itself, status); an exact slot that gives up returns the rows
    it did produce."""
    proto, n, R, exact = int(slot["protocol"]), int(slot["length"]), int(slot["rows"]), bool(slot["exact"])
    if proto == 0:
        ns = int(slot["n_sel"])
        idx = uniform_indices(ns, R, slot["seed"]) if (ns > 0 and R > 0) else np.zeros(0, np.int64)
        if ns == 0:
            idx = np.zeros(0, np.int64)
    elif proto == 4:
        kept = np.nonzero(occlusion_keep(slot, pts, normals))[0][:R]
        idx = kept
        if exact and 0 < len(kept) < R:
            idx = np.tile(kept, -(-R // len(kept)))[:R]
    else:
        prob = probabilities(slot, pts, normals)
        out, have = [], 0
        for t in range(MAX_PASSES if exact else 1):
            acc = np.nonzero(draws(slot["seed"], t, n) < prob)[0][:R - have]
            out.append(acc)
            have += len(acc)
            if have >= R or have == 0:
                break
        idx = np.concatenate(out) if out else np.zeros(0, np.int64)
    st = OK
    if exact and len(idx) < R:
        st = NO_POINT if len(idx) == 0 else PASS_BOUND
    return idx.astype(np.int64), st


def run_plan(slots, store_pts, store_normals, out_rows):
    """-> dict(src [out_rows] (-1 = a row the kernel leaves untouched), bids, pts [out_rows,3], counts [S], status [S])."""
    store_pts = np.asarray(store_pts, F)
    src = np.full(out_rows, -1, np.int64)
    bids = np.full(out_rows, -1, np.int64)
    counts = np.zeros(len(slots), np.int64)
    status = np.zeros(len(slots), np.int64)
    rot = np.zeros((out_rows, 9), F)
    for k, s in enumerate(slots):
        o, n, R, b = int(s["offset"]), int(s["length"]), int(s["rows"]), int(s["out_base"])
        nr = None if store_normals is None else store_normals[o:o + n]
        idx, st = select(s, store_pts[o:o + n], nr)
        counts[k], status[k] = len(idx), st
        rows = idx
        if st != OK:
            rows = np.concatenate([idx, np.zeros(R - len(idx), np.int64)])   # the model's row 0
        src[b:b + len(rows)] = o + rows
        bids[b:b + len(rows)] = int(s["batch_id"])
        rot[b:b + len(rows)] = s["rot"].astype(F)
    w = src >= 0
    p = store_pts[np.where(w, src, 0)]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.stack([x * rot[:, 0] + y * rot[:, 3] + z * rot[:, 6], x * rot[:, 1] + y * rot[:, 4] + z * rot[:, 7],
                    x * rot[:, 2] + y * rot[:, 5] + z * rot[:, 8]], axis=1).astype(F)
    return {"src": src, "bids": bids, "pts": out, "counts": counts, "status": status, "written": w}
