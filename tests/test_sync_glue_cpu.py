"""The dense glue with batch statistics across ranks, without a GPU: the NumPy model of the split (tests/sync_glue_ref.py)
meets the GPU tests' bar against the float64 whole-batch reference, gather_rows returns the rows bit for bit on both of its
routes, and the helper layers keep today's paths wherever the new op does not apply."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bn_act_ref as ref  # noqa: E402
import helpers  # noqa: E402
import sync_glue_ref as sref  # noqa: E402

SEED = 77
IDS = ["%dx%d" % s for s in sref.SHAPES]


# ------------------------------------------------------------------------------------------------- the model
_MODEL = {}


def _model(shape, relu, keepProb):
    key = (shape, relu, keepProb)
    if key not in _MODEL:
        _MODEL[key] = sref.model_forward(shape, relu, keepProb, SEED)
    return _MODEL[key]


def _whole(shape, relu, keepProb):
    d = sref.case(*shape)
    T = sref.threshold(keepProb)
    mask = None if keepProb is None else sref.keep_mask(SEED, shape[0], shape[1], T)
    scale = 1.0 if keepProb is None else float(np.float32(1.0) / np.float32(keepProb))
    return d, ref.forward(d["x"], d["gamma"], d["beta"], d["mov_mean"], d["mov_var"], True, relu, mask, scale), mask, scale


@pytest.mark.parametrize("shape", sref.SHAPES, ids=IDS)
def test_splits_cover_the_cases(shape):
    assert sref.bounds(shape)[-1][1] == shape[0] and min(sref.SPLITS[shape]) >= 1
    assert shape in ref.SHAPES


@pytest.mark.parametrize("shape", sref.SHAPES, ids=IDS)
def test_merged_rank_partials_meet_the_bar_where_the_f32_sum_of_squares_does_not(shape):
    d, out, _, _ = _whole(shape, False, None)
    m = _model(shape, False, None)
    assert m["N"] == shape[0] and m["bases"] == [a for a, _ in sref.bounds(shape)]
    helpers.assert_float_close(m["mean"], out["mean"], what="mean")
    helpers.assert_float_close(m["rstd"], out["rstd"], what="rstd")
    helpers.assert_float_close(m["mov_mean"], out["mov_mean"], what="moving mean")
    helpers.assert_float_close(m["mov_var"], out["mov_var"], what="moving variance")
    naive = ref.naive_f32_rstd(d["x"])                          # what the torch path's var = s2 / n - mean^2 gives
    assert np.abs(naive - out["rstd"]).max() / np.abs(out["rstd"]).max() > 1e-4


@pytest.mark.parametrize("relu,keepProb", [(False, None), (True, 0.7), (False, 0.7)], ids=["linear", "relu-drop", "linear-drop"])
@pytest.mark.parametrize("shape", sref.SHAPES, ids=IDS)
def test_model_forward_and_backward_meet_the_bar(shape, relu, keepProb):
    d, out, mask, scale = _whole(shape, relu, keepProb)
    m = _model(shape, relu, keepProb)
    helpers.assert_float_close(m["y"], out["y"], what="y")
    if keepProb is not None and not relu:
        # the mask of the concatenation is the whole batch's: the zeros an all-kept y could not have
        y = sref.model_forward(shape, False, keepProb, SEED)["y"]
        assert np.array_equal((y == 0) & (out["pre"] != 0), ~mask & (out["pre"] != 0))
    dx, dgs, dbs = sref.model_backward(shape, m, relu, keepProb, SEED)
    rdx, rdg, rdb = ref.backward(d["x"], d["dy"], d["gamma"], d["beta"], out["mean"], out["rstd"], relu, mask, scale,
                                 gate=m["gates"] if relu else None)
    helpers.assert_float_close(dx, rdx, what="dx")
    helpers.assert_float_close(np.sum(np.asarray(dgs, np.float64), 0), rdg, what="sum of dgamma")
    helpers.assert_float_close(np.sum(np.asarray(dbs, np.float64), 0), rdb, what="sum of dbeta")


# ------------------------------------------------------------------------------------------------- gather_rows
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(world, k):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((world, k)).astype(np.float32)
    a[0, 0], a[1, 1], a[0, 2] = -0.0, 0.0, np.float32(1e-42)   # a negative zero, a zero, a subnormal
    return a


def _gather_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mccnn_amd.dist import gather_rows
        want = _rows(world, 9)
        out = {}
        for route in ("reduce", None, "gather"):
            buf = torch.zeros(world, 9)
            buf[rank] = torch.from_numpy(want[rank])
            try:
                got = gather_rows(buf, route=route)
                out[route] = (got.data_ptr() == buf.data_ptr(), got.numpy().copy())
            except RuntimeError as err:                      # a backend without this collective on these tensors
                if route != "gather":
                    raise
                out[route] = str(err)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_gather_rows_over_two_gloo_ranks_is_exact_on_both_routes():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = _rows(world, 9)
    # a row that crossed the all-reduce has had +0.0 added to it: every bit but the sign of a zero
    def same(a, b, signed_zero):
        a, b = a.view(np.uint32), b.view(np.uint32)
        return np.array_equal(a, b) if signed_zero else np.array_equal(np.where(a == 0x80000000, 0, a), np.where(b == 0x80000000, 0, b))
    refused = [r for r in range(world) if isinstance(res[r]["gather"], str)]
    for r in range(world):
        for route in ("reduce", None):
            in_place, got = res[r][route]
            assert in_place and same(got, want, False), (r, route)
            assert got.view(np.uint32)[0, 2] == want.view(np.uint32)[0, 2]        # the subnormal came through
    if refused:
        assert len(refused) == world
        pytest.skip("gloo refuses all_gather_into_tensor here: %s" % res[0]["gather"][:200])
    for r in range(world):
        in_place, got = res[r]["gather"]
        assert in_place and same(got, want, True), r


def test_gather_rows_without_a_process_group_returns_the_buffer():
    from mccnn_amd.dist import gather_rows
    assert not dist.is_initialized()
    buf = torch.arange(6.0).reshape(1, 6)
    assert gather_rows(buf) is buf


# ------------------------------------------------------------------------------------------------- helpers
def test_store_switch_and_defaults():
    import mccnn_amd.MCNetworkUtils as U
    st = U.VariableStore()
    assert st.fusedSync_ is False and st.syncGroup_ is None and st.fused_ is False
    st = U.VariableStore(None, True, True, True)
    assert st.fused_ and st.fusedLinear_ and st.fusedSync_
    st.fusedSync_ = False
    assert list(st.state_dict().keys()) == []                   # switches are no state


def test_fused_sync_on_cpu_tensors_without_a_group_takes_the_torch_path():
    import mccnn_amd.MCNetworkUtils as U
    torch.manual_seed(3)
    x = torch.randn(40, 6)
    outs = []
    for kw in (dict(), dict(fused=True, fusedSync=True)):
        st = U.VariableStore(**kw)
        assert U._fused_glue(st, x, True, "L_BN", True, 0.7) is None     # a CPU tensor: never the library op
        xx = x.clone().requires_grad_(True)
        y = U.batch_norm_RELU_drop_out("L", xx, True, False, None, st)
        y.sum().backward()
        outs.append((y.detach().numpy().tobytes(), xx.grad.numpy().tobytes(), list(st.state_dict().keys()), st.dropCalls_,
                     st.state_dict()["L_BN/moving_mean"].numpy().tobytes()))
    assert outs[0] == outs[1]


def _cpu_glue_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import mccnn_amd.MCNetworkUtils as U
        torch.manual_seed(0)
        full = torch.randn(50, 4) * 2 + 0.5
        part = full[:20] if rank == 0 else full[20:]
        outs = []
        for kw in (dict(), dict(fused=True, fusedSync=True)):
            st = U.VariableStore(**kw)
            assert U._fused_glue(st, part, True, "L_BN", True, None) is None      # CPU tensors in a group of two ranks
            xx = part.clone().requires_grad_(True)
            y = U.batch_norm_RELU_drop_out("L", xx, True, False, None, st)
            (y * y).sum().backward()
            outs.append((y.detach().numpy().tobytes(), xx.grad.numpy().tobytes(), st.dropCalls_))
        q.put((rank, outs[0] == outs[1]))
    finally:
        dist.destroy_process_group()


def test_fused_sync_on_cpu_tensors_in_a_group_takes_the_torch_sync_path():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_cpu_glue_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == {0: True, 1: True}


def test_abi_declares_the_four_stages():
    from mccnn_amd import _lib
    lib = _lib.load()
    assert lib.mccnn_abi_version() >= 22
    for name in ("mccnn_bn_sync_stats", "mccnn_bn_sync_apply", "mccnn_bn_sync_bwd_sums", "mccnn_bn_sync_bwd_dx"):
        assert hasattr(lib, name)
    header = open(os.path.join(os.path.dirname(HERE), "include", "mccnn.h")).read()
    for name in ("mccnn_bn_sync_stats", "mccnn_bn_sync_apply", "mccnn_bn_sync_bwd_sums", "mccnn_bn_sync_bwd_dx"):
        assert "int %s(" % name in header


def test_argument_errors_come_before_any_launch():
    """The checks need no GPU: every refused call returns before it touches a pointer."""
    from mccnn_amd import _lib
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    p = 4096                                                    # never dereferenced
    assert lib.mccnn_bn_sync_stats(p, 0, 300, 8, 2, 2, p, p, 1 << 20, None) == -1          # rank == world
    assert lib.mccnn_bn_sync_stats(p, 0, 300, 8, -1, 2, p, p, 1 << 20, None) == -1
    assert lib.mccnn_bn_sync_stats(p, 0, 300, 8, 0, 0, p, p, 1 << 20, None) == -1          # world < 1
    assert lib.mccnn_bn_sync_stats(p, 0, (1 << 24) + 1, 8, 0, 2, p, p, 1 << 40, None) == -3
    assert lib.mccnn_bn_sync_stats(p, 0, 1 << 24, 8, 0, 2, p, p, 16, None) == -4           # 2^24 rows pass that check
    assert lib.mccnn_bn_sync_stats(None, 0, 300, 8, 0, 2, p, p, 1 << 20, None) == -1
    assert lib.mccnn_bn_sync_stats(p, 0, 300, 8, 0, 2, None, p, 1 << 20, None) == -1
    assert lib.mccnn_bn_sync_stats(p, 2, 300, 8, 0, 2, p, p, 1 << 20, None) == -1          # a type flag outside {0, 1}
    assert lib.mccnn_bn_sync_stats(p, 0, 300, 8, 0, 2, p, None, 0, None) == -4
    assert lib.mccnn_bn_sync_stats(p, 0, 300, 8, 0, 2, p, p, 8, None) == -4
    assert lib.mccnn_bn_sync_stats(p, 1, 300, 7, 0, 2, p, p, 1 << 20, None) == -5          # bf16 rows, odd c
    assert lib.mccnn_debug_launch_count() == before
