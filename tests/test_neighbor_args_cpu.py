"""Argument checks of the six mccnn_find_neighbors_* entries without a GPU: 162 calls that must return before any launch --
negative sizes, a zero or NaN radius, every null pointer with n = 0 and n > 0, a missing or short workspace, e < 0 and = 0,
m = 0, caps of -1 and 0 -- against the codes recorded in tests/golden/neighbor_badarg_codes.txt (taken from the library as it
was before the entries were routed through one NeighSearch record: the checks, their order and their codes are part of the
interface)."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _codes(lib):
    i, f, sz, u, vp = C.c_int, C.c_float, C.c_size_t, C.c_uint, C.c_void_p
    buf = (C.c_char * 65536)()
    p = C.cast(buf, C.c_void_p)
    N = C.c_void_p(None)
    common = [vp, vp, i, vp, i, vp, vp, vp, i, i, f, i, vp]
    sigs = {
        "mccnn_find_neighbors_count": common + [vp, vp, vp, sz, vp],
        "mccnn_find_neighbors_count2": common + [vp, vp, vp, vp, sz, vp],
        "mccnn_find_neighbors_fill": common + [vp, i, vp, vp, sz, vp],
        "mccnn_find_neighbors_count_capped": common + [vp, vp, vp, sz, vp, i],
        "mccnn_find_neighbors_fill_capped": common + [vp, i, vp, vp, sz, vp, i],
        "mccnn_find_neighbors_fill_sampled": common + [vp, i, vp, vp, sz, vp, i, u],
    }
    for k, s in sigs.items():
        getattr(lib, k).argtypes, getattr(lib, k).restype = s, i
    def base(m=10, n=10, B=1, nc=2, r=0.5):
        return [p, p, m, p, n, p, p, p, B, nc, r, 0, N]
    out = []
    def run(name, args, tag):   # (only calls that return before any launch: bad arguments, workspace too small, nothing to do)
        out.append("%s %s -> %d" % (name, tag, getattr(lib, name)(*args)))
    for name in sigs:
        fill = "fill" in name
        tailv = [4, 9] if name.endswith("sampled") else ([4] if name.endswith("capped") else [])   # max_neighbors, seed
        def mk(b, start=p, total=p, e=5, packed=p, ws=p, wsb=16, tail=None):
            t = tailv if tail is None else tail
            if fill: return b + [start, e, packed, ws, wsb, N] + t
            if name.endswith("count2"): return b + [start, total, N, ws, wsb, N] + t
            return b + [start, total, ws, wsb, N] + t
        for tag, kw in [("m<0", dict(m=-1)), ("n<0", dict(n=-1)), ("B0", dict(B=0)), ("nc0", dict(nc=0)), ("r0", dict(r=0.0)), ("rnan", dict(r=float("nan")))]:
            run(name, mk(base(**kw)), tag)
        # (every case passes a 16-byte workspace unless it says otherwise: a call whose arguments pass the checks ends at the
        # workspace check, before any launch -- "ws small" is that baseline, all arguments valid)
        run(name, mk(base(), wsb=16), "ws small")
        run(name, mk(base(), ws=N), "ws null")
        run(name, mk(base(), start=N), "start null")
        run(name, mk(base(), start=N, wsb=16, e=0), "start null e0")
        for idx in (0, 1, 3, 5, 6, 7):
            b = base(); b[idx] = N
            run(name, mk(b), "null arg %d" % idx)
            b = base(n=0); b[idx] = N
            run(name, mk(b), "null arg %d n0" % idx)
        if fill:
            run(name, mk(base(), e=-1), "e<0")
            run(name, mk(base(), e=0, ws=N), "e0")
            run(name, mk(base(m=0), ws=N), "m0")
            run(name, mk(base(), packed=N), "packed null")
        else:
            run(name, mk(base(), total=N), "total null")
            run(name, mk(base(m=0), total=N), "m0 total null")
        if tailv:
            for t0 in (-1, 0):
                run(name, mk(base(), tail=[t0] + tailv[1:]), "K=%d" % t0)
                run(name, mk(base(), tail=[t0] + tailv[1:], ws=N), "K=%d ws null" % t0)
    return out


def test_bad_argument_calls_return_the_recorded_codes():
    from mccnn_amd import build
    got = _codes(C.CDLL(build.build()))   # (a handle of its own: plain pointer-sized argument types)
    want = open(os.path.join(ROOT, "tests", "golden", "neighbor_badarg_codes.txt")).read().split("\n")
    want = [w for w in want if w]
    assert len(got) == len(want) == 162
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:5]
    assert {g.rsplit(" ", 1)[1] for g in got} == {"-1", "-4", "0"}   # bad argument, workspace, nothing to do: no launch was reached
