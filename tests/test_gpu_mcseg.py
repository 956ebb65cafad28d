"""examples/mcseg.py on the GPU: MCSeg(1, 4, 8, numCats, numParts) on modelnet_like(1024, 4, 51), whose hierarchy
[0.025, 0.1, 0.4] has levels above and below 256 points, so the glue over a concatenation runs in its two-launch and its
one-launch form. (a) every fused glue switch on against all off, (b) both against the CPU twin (oracle ops, stock torch
glue; the three nets are computed once and shared by (a) and (b)), (c) the variable names under every flag combination, (d) the full dropout as a function of (dropSeed_, dropCalls_)."""
import itertools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "examples"))

NUM_CATS, NUM_PARTS, K, B, N = 3, 6, 8, 4, 1024


def _batch(dev):
    import torch
    from mccnn_amd.workloads import modelnet_like
    pts, bids = modelnet_like(N, B, 51)
    y = np.random.default_rng(2).integers(0, NUM_PARTS, len(pts))
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    P, Bi = t(pts), t(bids)
    return P, Bi, torch.ones((len(pts), 1), device=dev), (Bi.reshape(-1) % NUM_CATS).long(), t(y)


def _switch(net, on):
    net.store.fused_ = net.store.fusedCat_ = net.fusedLinear = on   # (MCSeg's fusedLinear: the conv_1x1 + _Out_BN pairs)


def _run(net, dev):
    """Forward + loss + backward, conv and full dropout off -> (logits, loss, gradients by name, state_dict, level sizes)."""
    import torch
    for p in net.parameters():
        p.grad = None
    P, Bi, F, cats, y = _batch(dev)
    logits = net(P, Bi, F, cats, True, useDropOutFull=False)
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    named = dict(net.convBuilder.named_parameters())
    named.update(dict(net.store.named_parameters()))
    assert all(v.grad is not None for v in named.values())
    return (logits.detach().cpu().numpy(), float(loss.detach()), {k_: v.grad.detach().cpu().numpy() for k_, v in named.items()},
            {k_: v.detach().cpu().numpy() for k_, v in net.state_dict().items()}, [int(p.shape[0]) for p in net.lastHierarchy.points_])


def _errors(got, want):
    """Per quantity: the logits and every gradient relative to the largest entry of the reference (gradients: never below
    1e-3 of the largest gradient entry of all, the floor of test_mcclass_s_fused_matches_the_cpu_twin), the loss relative."""
    (gl, gloss, gg, _, _), (cl, closs, cg, _, _) = got, want
    gmax = max(float(np.abs(v).max()) for v in cg.values())
    err = {"grad " + k_: float(np.abs(gg[k_] - cg[k_]).max() / max(np.abs(cg[k_]).max(), 1e-3 * gmax)) for k_ in cg}
    err["logits"] = float(np.abs(gl - cl).max() / max(np.abs(cl).max(), 1e-30))
    err["loss"] = abs(gloss - closs) / abs(closs)
    return err


def _worst(err):
    k_ = max((k for k in err if k.startswith("grad ")), key=err.get)
    return "logits %.1e loss %.1e worst gradient %.1e (%s) over %d tensors" % (err["logits"], err["loss"], err[k_], k_[5:], len(err) - 2)


_RES = {}


def _results():
    """The fused-off GPU net, the fused-on one (fused + fusedCat + fusedLinear) and the CPU twin (oracle ops, stock torch glue)
    on the same weights and batch, conv and full dropout off; computed once and shared (read-only)."""
    if not _RES:
        import torch
        from mcseg import MCSeg
        from oracle.oracle import Oracle
        from tests.oracle_ops import OracleOps
        dev = torch.device("cuda", 0)
        torch.manual_seed(3)
        gnet = MCSeg(1, B, K, NUM_CATS, NUM_PARTS, dev)
        with torch.no_grad():
            gnet(*_batch(dev)[:4], True, useDropOutFull=False)     # creates the variables, every switch off
        cnet = MCSeg(1, B, K, NUM_CATS, NUM_PARTS, torch.device("cpu"), ops=OracleOps(Oracle(omp=True)))
        cnet.load_state_dict({k_: v.detach().cpu().clone() for k_, v in gnet.state_dict().items()})
        start = {k_: v.detach().clone() for k_, v in gnet.state_dict().items()}
        for tag in ("off", "on"):
            gnet.load_state_dict(start)                              # (the moving statistics of the run before)
            _switch(gnet, tag == "on")
            _RES[tag] = _run(gnet, dev)
        assert gnet.store.dropCalls_ == 0                            # no block dropped
        _RES["cpu"] = _run(cnet, torch.device("cpu"))
        levels = _RES["cpu"][4]
        print("levels %s" % levels)
        assert levels == [4096, 3174, 680, 35]                      # (the oracle's hierarchy of this input)
        assert _RES["off"][4] == levels and _RES["on"][4] == levels
        assert max(levels[1:]) > 256 >= min(levels[1:])             # the glue runs in both forms
    return _RES


def test_mcseg_fused_glue_on_matches_off(mc):
    """(a) fused + fusedCat + fusedLinear on against all off, same weights and batch: the bars and the scale floor of
    test_mcclass_s_fused_matches_the_cpu_twin -- logits and every parameter gradient 1e-4 (a gradient's scale never below 1e-3 of
    the largest gradient entry of all), loss 1e-5.

    Observed on an MI355X: logits 2.7e-07, loss 0.0e+00 (the same float), worst gradient 6.8e-05 (Reduce_Pool_1_biases, whose
    exact value is zero: a bias in front of a batch norm) over 146 tensors."""
    res = _results()
    ea = _errors(res["on"], res["off"])
    print("fused on vs off: " + _worst(ea))
    assert set(res["on"][2]) == set(res["off"][2])
    over = {k_: e for k_, e in ea.items() if e > (1e-5 if k_ == "loss" else 1e-4)}
    for k_, e in sorted(over.items()):
        print("  over its bar: %s %.2e" % (k_, e))
    assert not over, over


def test_mcseg_both_gpu_nets_match_the_cpu_twin(mc):
    """(b) both GPU nets against the CPU twin. The fused-off net is torch.cat + torch glue, and what it shows against the twin
    sets the fused net's bar: per quantity (logits, loss, every gradient, the moving statistics) max(1e-4, 2 x that error),
    both measured here on the same batch; the factor 2 allows for the other summation order of the statistics.

    Observed on an MI355X, fused off and fused on alike: logits 3.3e-06, loss 1.1e-07, worst gradient 3.2e-04
    (DeConv_1_Reduce_In_BN_BN/beta) over 146 tensors; no quantity of the fused net outside its bar."""
    res = _results()
    e_off, e_on = _errors(res["off"], res["cpu"]), _errors(res["on"], res["cpu"])
    print("fused off vs twin: " + _worst(e_off))
    print("fused on  vs twin: " + _worst(e_on))
    over = {k_: (e_on[k_], e_off[k_]) for k_ in e_off if e_on[k_] > max(1e-4, 2.0 * e_off[k_])}
    for k_, (e1, e0) in sorted(over.items()):
        print("  over its bar: %s on %.2e off %.2e" % (k_, e1, e0))
    assert not over, over
    worst = {}
    for tag in ("off", "on"):
        gsd, csd = res[tag][3], res["cpu"][3]
        assert set(gsd) == set(csd)
        moving = [k_ for k_ in csd if k_.endswith("/moving_mean") or k_.endswith("/moving_variance")]
        assert len(moving) == 44                                 # 22 batch-norm blocks
        smax = max(float(np.abs(csd[k_]).max()) for k_ in moving)
        worst[tag] = max(float(np.abs(gsd[k_] - csd[k_]).max() / max(np.abs(csd[k_]).max(), 1e-3 * smax)) for k_ in moving)
        print("moving statistics, fused %s vs twin: %.1e" % (tag, worst[tag]))
    assert worst["on"] <= max(1e-4, 2.0 * worst["off"])


def test_mcseg_variable_names_do_not_depend_on_the_switches(mc):
    """(c) state_dict keys and their order under every combination of fused, fusedCat, fusedLinear and fusedLoss."""
    import torch
    from mcseg import MCSeg
    dev = torch.device("cuda", 0)
    P, Bi, F, cats, y = _batch(dev)
    keys = None
    for fused, fusedCat, fusedLinear, fusedLoss in itertools.product((False, True), repeat=4):
        net = MCSeg(1, B, K, NUM_CATS, NUM_PARTS, dev, fused=fused, fusedCat=fusedCat, fusedLinear=fusedLinear, fusedLoss=fusedLoss)
        with torch.no_grad():
            out = net(P, Bi, F, cats, True, labels=y if fusedLoss else None)
        assert (tuple(out.shape) == (B * N, NUM_PARTS)) if not fusedLoss else (out.loss.dim() == 0)
        got = list(net.state_dict().keys())
        keys = keys or got
        assert got == keys, (fused, fusedCat, fusedLinear, fusedLoss)
    moving = [k_ for k_ in keys if k_.endswith("/moving_mean") or k_.endswith("/moving_variance")]
    assert len(moving) == 2 * MCSeg.NUM_BN_BLOCKS == 44
    for name in ("store.Reduce_Pool_2_In_BN_BN/gamma", "store.Up_3_4_BN_BN/beta", "store.DeConv_3_Reduce_In_BN_BN/moving_mean",
                 "store.DeConv_1_Reduce_weights", "store.Final_Logits_BN_h1/gamma"):
        assert name in keys, name
    assert tuple(net.state_dict()["store.DeConv_1_Reduce_In_BN_BN/gamma"].shape) == (13 * K,)
    assert tuple(net.state_dict()["store.DeConv_3_Reduce_In_BN_BN/gamma"].shape) == (24 * K,)


def test_mcseg_full_dropout_is_a_function_of_the_seed_and_the_counter(mc):
    """(d) as in the MCClassS test: with the full dropout on, the logits depend on (dropSeed_, dropCalls_) alone."""
    import torch
    from mcseg import MCSeg
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    net = MCSeg(1, B, K, NUM_CATS, NUM_PARTS, dev, fused=True, fusedCat=True, fusedLinear=True)
    P, Bi, F, cats, _ = _batch(dev)

    def logits_at(seed, calls):
        net.store.dropSeed_, net.store.dropCalls_ = seed, calls
        with torch.no_grad():
            out = net(P, Bi, F, cats, True, useDropOutFull=True)
        assert net.store.dropCalls_ == calls + 2                # the two hidden layers of Final_Logits dropped
        return out.cpu().numpy()

    with torch.no_grad():
        net(P, Bi, F, cats, True)                               # creates the variables
    a, b, c = logits_at(4, 0), logits_at(4, 0), logits_at(5, 7)   # (training forwards move the statistics, not the logits)
    assert a.tobytes() == b.tobytes()
    assert not np.array_equal(a, c)
