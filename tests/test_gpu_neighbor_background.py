"""find_neighbors as a background launch (mccnn_background_launches(1) on the calling thread): the single-launch kernels
with the plain candidate loop, which the foreground calls of every other test file never take (theirs are the lean loop).
startIndexs and packedNeighs byte for byte against the same call without the flag, and against the oracle's uncapped list
thinned by tests/neighbor_cap_ref.py (canonical ranks) or tests/neighbor_sample_ref.py (a seed).

Geometries of tests/neighbor_cap_ref.py: `mixed` (1020 centres; under the absolute radius windows of up to 586 points: all
three window regimes of the kernel) uncapped and at K = 16 in both radius modes, `big_windows` (3000 centres, windows of up
to 1056 points) at K = 64; every capped case canonical and with sampleSeed = 7."""
import numpy as np
import pytest

from tests import neighbor_sample_ref as ref

pytestmark = pytest.mark.gpu

_ORACLE_LISTS = {}   # (geometry name, scaleInv) -> (geometry, the oracle's uncapped chain): computed once, never modified
_GRIDS = {}          # the same key -> the GPU's grid of that geometry

CASES = [(name, si, K, seed)
         for name, si, K in (("mixed", True, 0), ("mixed", False, 0), ("mixed", True, 16), ("mixed", False, 16),
                             ("big_windows", True, 64))
         for seed in ((None,) if K == 0 else (None, 7))]


def _wrap(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unwrap(t):
    return t.detach().cpu().numpy()


def _setup(mc, oracle, name, scaleInv):
    key = (name, scaleInv)
    if key not in _ORACLE_LISTS:
        g = dict(ref.GEOMETRIES[name](), scaleInv=scaleInv)
        _ORACLE_LISTS[key] = (g, ref.uncapped(oracle, g))
        P, Bi = _wrap(g["pts"]), _wrap(g["bids"])
        mn, mx = mc.compute_aabb(P, Bi, g["B"], scaleInv)
        sP, sB, cells, idx, inv = mc.build_grid(P, Bi, mn, mx, g["B"], g["radius"], scaleInv)
        _GRIDS[key] = dict(mn=mn, mx=mx, sP=sP, cells=cells, C=_wrap(g["centres"]), Cb=_wrap(g["cbids"]))
    return _ORACLE_LISTS[key] + (_GRIDS[key],)


def _search(mc, g, h, K, seed, background):
    from mccnn_amd import _lib
    kw = {} if seed is None else {"sampleSeed": seed}
    lib = _lib.load()
    prev = lib.mccnn_background_launches(1) if background else 0
    try:
        return mc.find_neighbors(h["C"], h["Cb"], h["sP"], h["cells"], h["mn"], h["mx"], g["radius"], g["B"], g["scaleInv"],
                                 maxNeighbors=K, **kw)
    finally:
        if background:
            lib.mccnn_background_launches(prev)


@pytest.mark.parametrize("name,scaleInv,K,seed", CASES)
def test_background_search_equals_foreground_and_oracle(mc, oracle, name, scaleInv, K, seed):
    g, r, h = _setup(mc, oracle, name, scaleInv)
    assert np.array_equal(_unwrap(h["sP"]), r["sortPts"]) and np.array_equal(_unwrap(h["cells"]), r["cellIndexs"])
    if seed is None:
        st, pk = ref.cap_list(r["startIndexs"], r["packedNeighs"], K)
    else:
        st, pk = ref.sample_list(r["startIndexs"], r["packedNeighs"], K, seed)
    w = ref.window_sizes(g, r)
    if name == "mixed":
        assert len(w) == 1020
        if not scaleInv:   # all three window regimes in one list
            assert (w <= 256).any() and ((w > 256) & (w <= 512)).any() and (w > 512).any() and w.max() == 586
    else:
        assert len(w) == 3000 and w.max() == 1056
    bg_st, bg_pk = _search(mc, g, h, K, seed, True)
    fg_st, fg_pk = _search(mc, g, h, K, seed, False)
    bg_st, bg_pk, fg_st, fg_pk = _unwrap(bg_st), _unwrap(bg_pk), _unwrap(fg_st), _unwrap(fg_pk)
    assert bg_st.dtype == fg_st.dtype == st.dtype and bg_pk.dtype == fg_pk.dtype == pk.dtype
    assert bg_st.shape == fg_st.shape and bg_st.tobytes() == fg_st.tobytes(), "startIndexs: background != foreground"
    assert bg_pk.shape == fg_pk.shape and bg_pk.tobytes() == fg_pk.tobytes(), "packedNeighs: background != foreground"
    assert bg_st.shape == st.shape and bg_st.tobytes() == st.tobytes(), "startIndexs: background != thinned oracle list"
    assert bg_pk.shape == pk.shape and bg_pk.tobytes() == pk.tobytes(), "packedNeighs: background != thinned oracle list"
