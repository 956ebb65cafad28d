"""Voxel accuracy on the GPU (mccnn_voxel_acc_add, MCConvModule.voxel_counts, native.voxel_counts, MCNetworkUtils.voxel_counts
with VariableStore(fusedLoss=True)) against the NumPy model of tests/voxel_acc_ref.py. Every comparison of counts, and of
the rows dropped, is exact integer equality."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import voxel_acc_ref as ref  # noqa: E402

ROUTES = ("abi", "glue", "native", "helper")


def _dev(a, offset=False):
    """`a` on the GPU; offset: as a contiguous view that starts 4 bytes into its buffer."""
    import torch
    if a is None:
        return None
    t = torch.from_numpy(np.array(a)).to(torch.device("cuda", 0))
    if not offset:
        return t
    flat = t.reshape(-1)
    buf = torch.zeros(flat.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = flat
    v = buf[1:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() - buf.data_ptr() == 4 and v.data_ptr() % 16 == 4
    return v


def _zeros(d):
    import torch
    return torch.zeros((d["B"], d["C"], 2), dtype=torch.int64, device=torch.device("cuda", 0))


def _table(d, slots=None):
    """A zeroed workspace of the recommended size, or of exactly `slots` slots."""
    import torch
    from mccnn_amd import _lib
    nbytes = _lib.load().mccnn_voxel_acc_workspace_bytes(d["n"], d["C"]) if slots is None else slots * (8 + 8 * d["C"])
    return torch.zeros(nbytes, dtype=torch.uint8, device=torch.device("cuda", 0))


def _abi(d, t, out, dropped, ws, clean):
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    _lib.check(lib.mccnn_voxel_acc_add(t["points"].data_ptr(), t["pred"].data_ptr(), t["labels"].data_ptr(), _lib.ptr(t["bid"]),
                                       t["mn"].data_ptr(), d["n"], d["B"], d["C"], d["ignore"], float(d["res"]), d["share"],
                                       out.data_ptr(), _lib.ptr(dropped), ws.data_ptr(), ws.numel(), clean, _lib.stream_handle()),
               "voxel_acc_add")
    return lib.mccnn_debug_launch_count() - before


def _tensors(d, offset=False):
    t = {k: _dev(d[k]) for k in ("points", "mn")}
    t.update({k: _dev(d[k], offset) for k in ("pred", "labels", "bid")})
    return t


def _add(route, d, out, dropped=None, offset=False):
    """One call of `route` over case `d` into the device tensors `out`, `dropped` -> library launches."""
    import torch
    import mccnn_amd.MCConvModule as M
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib, native
    lib = _lib.load()
    t = _tensors(d, offset)
    if route == "abi":
        launches = _abi(d, t, out, dropped, _table(d), 0) - 1            # (the clear of ws_clean = 0)
    else:
        kw = dict(resolution=d["res"], ignoreLabel=d["ignore"], maxIgnoreShare=d["share"], out=out, dropped=dropped)
        before = lib.mccnn_debug_launch_count()
        if route == "helper":
            head = U.LossHead(None, t["pred"], None, None, None)
            got = U.voxel_counts(t["points"], head, t["labels"], d["C"], t["bid"], d["B"], t["mn"], store=U.VariableStore(fusedLoss=True), **kw)
        else:
            op = M.voxel_counts if route == "glue" else native.voxel_counts
            got = op(t["points"], t["pred"], t["labels"], d["C"], t["bid"], d["B"], t["mn"], **kw)
        assert got is out
        launches = lib.mccnn_debug_launch_count() - before
    torch.cuda.synchronize()
    return launches


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_counts_equal_the_model(mc, name, route):
    """Every case through the C-ABI, the ctypes op, the extension op and the helper (fusedLoss on, a LossHead as pred): two
    launches (vote, score), the model's counts and its dropped rows exactly."""
    import torch
    d, want, wdrop = ref.case(name)
    out = _zeros(d)
    dropped = torch.full((1,), 7, dtype=torch.int32, device=out.device)
    assert _add(route, d, out, dropped) == 2
    got = out.cpu().numpy()
    print("%s/%s: n %d, V %d G %d, dropped %d" % ((name, route, d["n"]) + tuple(got.sum((0, 1)).tolist()) + (int(dropped) - 7,)))
    assert np.array_equal(got, want)
    assert int(dropped) == 7 + wdrop
    if name == "dead-rows":
        assert wdrop > 0


@pytest.mark.parametrize("slots", [None, 4096], ids=["recommended", "cap-min"])
def test_4095_voxels_in_a_full_table(mc, slots):
    """4095 distinct voxels: with the recommended 8192 slots, and with exactly cap_min = 4096 slots -- a load of 0.9998, probe
    chains that wrap the table's end. A workspace one slot short of cap_min is refused; the table is all zero afterwards."""
    import torch
    from mccnn_amd import _lib
    d, want, _ = ref.case("distinct-4095")
    assert d["n"] == 4095 and int(want[:, :, 1].sum()) == 4095
    t = _tensors(d)
    ws = _table(d, slots)
    assert ws.numel() == (8192 if slots is None else 4096) * (8 + 8 * d["C"])
    out = _zeros(d)
    assert _abi(d, t, out, None, ws, 0) == 3
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert int(ws.to(torch.int32).sum()) == 0
    if slots is not None:
        lib = _lib.load()
        before = lib.mccnn_debug_launch_count()
        short = ws[:ws.numel() - 16]
        rc = lib.mccnn_voxel_acc_add(t["points"].data_ptr(), t["pred"].data_ptr(), t["labels"].data_ptr(), None, t["mn"].data_ptr(),
                                     d["n"], 1, d["C"], d["ignore"], float(d["res"]), d["share"], out.data_ptr(), None,
                                     short.data_ptr(), short.numel(), 0, _lib.stream_handle())
        assert rc == -4 and lib.mccnn_debug_launch_count() == before


@pytest.mark.parametrize("name", ["room", "dead-rows", "one-voxel-70000"])
def test_launch_counts_and_the_workspace_the_op_leaves(mc, name):
    """3 launches with ws_clean = 0 (on a workspace full of ones), 2 with ws_clean = 1 on the workspace the first call left,
    the same counts both times; the workspace read back after either call is all zero; n == 0 launches nothing."""
    import torch
    from mccnn_amd import _lib
    d, want, wdrop = ref.case(name)
    t = _tensors(d)
    ws = _table(d)
    ws.fill_(0xFF)
    first, second = _zeros(d), _zeros(d)
    dropped = torch.zeros(1, dtype=torch.int32, device=ws.device)
    assert _abi(d, t, first, dropped, ws, 0) == 3
    torch.cuda.synchronize()
    assert not bool(ws.any())
    assert _abi(d, t, second, dropped, ws, 1) == 2
    torch.cuda.synchronize()
    assert not bool(ws.any())
    assert np.array_equal(first.cpu().numpy(), want) and np.array_equal(second.cpu().numpy(), want)
    assert int(dropped) == 2 * wdrop
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    rc = lib.mccnn_voxel_acc_add(t["points"].data_ptr(), t["pred"].data_ptr(), t["labels"].data_ptr(), _lib.ptr(t["bid"]),
                                 t["mn"].data_ptr(), 0, d["B"], d["C"], d["ignore"], float(d["res"]), d["share"], first.data_ptr(),
                                 None, ws.data_ptr(), ws.numel(), 0, _lib.stream_handle())
    assert rc == 0 and lib.mccnn_debug_launch_count() == before
    torch.cuda.synchronize()
    assert np.array_equal(first.cpu().numpy(), want)


@pytest.mark.parametrize("route", ROUTES)
def test_views_that_start_four_bytes_into_their_buffers(mc, route):
    """pred, labels and batch ids as views 4 bytes into their buffers: the same counts."""
    d, want, _ = ref.case("dead-rows")
    out = _zeros(d)
    assert _add(route, d, out, offset=True) == 2
    assert np.array_equal(out.cpu().numpy(), want)
    d, want, _ = ref.case("room")
    out = _zeros(d)
    assert _add(route, d, out, offset=True) == 2
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize("route", ROUTES)
def test_accumulation_into_out(mc, route):
    """A second call adds: twice the counts; a start above 2^32 is kept."""
    import torch
    d, want, _ = ref.case("two-clouds")
    out = _zeros(d)
    _add(route, d, out)
    _add(route, d, out)
    assert np.array_equal(out.cpu().numpy(), 2 * want)
    start = np.full(want.shape, (1 << 40) + 5, np.int64)
    out = torch.from_numpy(start.copy()).to(out.device)
    _add(route, d, out)
    assert np.array_equal(out.cpu().numpy(), start + want)


def test_two_runs_give_the_same_bytes(mc):
    for name in ("room", "one-voxel-70000"):
        d, want, _ = ref.case(name)
        runs = []
        for _ in range(2):
            out = _zeros(d)
            _add("abi", d, out)
            runs.append(out.cpu().numpy().tobytes())
        assert runs[0] == runs[1] == want.tobytes()


def test_int64_inputs_a_fresh_result_and_the_kept_table(mc):
    """int64 pred / labels of shape (n, 1) are cast; out=None returns a zeroed tensor's counts; the ops' own table is kept
    between calls and is all zero after each."""
    import torch
    from mccnn_amd import dense_glue, native
    d, want, _ = ref.case("dead-rows")
    t = _tensors(d)
    for op in (mc.voxel_counts, native.voxel_counts):
        for _ in range(2):
            got = op(t["points"], t["pred"].to(torch.int64).reshape(-1, 1), t["labels"].to(torch.int64).reshape(-1, 1), d["C"],
                     t["bid"].reshape(-1, 1), d["B"], t["mn"], d["res"], d["ignore"], d["share"])
            assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    ws = dense_glue._voxel_ws(d["n"], d["C"], t["points"].device)
    assert ws.numel() == dense_glue.voxel_cap_rec(d["n"]) * (8 + 8 * d["C"]) and not bool(ws.any())
    assert dense_glue._voxel_ws(d["n"], d["C"], t["points"].device) is ws


@pytest.mark.parametrize("name", ["room", "dead-rows", "two-clouds", "planted-oob"])
def test_the_helper_with_the_switch_off_is_equal(mc, name):
    """MCNetworkUtils.voxel_counts on the same device tensors: two library launches with the switch on, none and the torch code
    of the same definition with it off -- the model's counts and dropped rows either way; the score on the device."""
    import torch
    import mccnn_amd.MCNetworkUtils as U
    from mccnn_amd import _lib
    lib = _lib.load()
    d, want, wdrop = ref.case(name)
    t = _tensors(d)
    res = {}
    for switch, launches in ((True, 2), (False, 0)):
        st = U.VariableStore(fusedLoss=switch)
        out = _zeros(d)
        dropped = torch.zeros(1, dtype=torch.int32, device=out.device)
        before = lib.mccnn_debug_launch_count()
        got = U.voxel_counts(t["points"], t["pred"], t["labels"], d["C"], t["bid"], d["B"], t["mn"], d["res"], d["ignore"], d["share"],
                             out=out, dropped=dropped, store=st)
        assert lib.mccnn_debug_launch_count() - before == launches and got is out
        res[switch] = (got.cpu().numpy(), int(dropped))
        assert np.array_equal(res[switch][0], want) and res[switch][1] == wdrop
    assert res[True][0].tobytes() == res[False][0].tobytes()
    s = U.voxel_scores(got, d["ignore"])
    acc, mean = ref.scores(want, d["ignore"])
    assert s.acc.is_cuda and np.abs(s.acc.cpu().numpy() - acc).max() <= 1e-12 and abs(float(s.meanAcc) - mean) <= 1e-12


@pytest.mark.parametrize("switch", [True, False], ids=["on", "off"])
def test_the_default_box(mc, switch):
    """aabbMin=None: compute_aabb's per-cloud minimum, bit-exact -- the room's own box, and the two clouds' boxes."""
    import mccnn_amd.MCNetworkUtils as U
    st = U.VariableStore(fusedLoss=switch)
    d, want, _ = ref.case("room")
    t = _tensors(d)
    got = U.voxel_counts(t["points"], t["pred"], t["labels"], d["C"], resolution=d["res"], ignoreLabel=0, store=st)
    assert np.array_equal(got.cpu().numpy(), want)
    d, _, _ = ref.case("two-clouds")
    t = _tensors(d)
    mins = np.stack([d["points"][d["bid"] == b].min(0) for b in range(2)])
    assert np.array_equal(U._box_min(t["points"], t["bid"], 2).cpu().numpy(), mins)
    wmin, _ = ref.model(d["points"], d["pred"], d["labels"], d["C"], mins, d["bid"], 2, d["res"], d["ignore"], d["share"])
    got = U.voxel_counts(t["points"], t["pred"], t["labels"], d["C"], t["bid"].reshape(-1, 1), 2, None, d["res"], d["ignore"], store=st)
    assert np.array_equal(got.cpu().numpy(), wmin)
