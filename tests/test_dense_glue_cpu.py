"""Where the dense glue lives (mccnn_amd/dense_glue.py) without a GPU: every name MCConvModule had for it is still there
and is dense_glue's own object, whichever of the two modules is imported first, and the three wrappers of mccnn_amd.native
still end in its checks."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bn_relu_dropout", "bn_relu_dropout_sync", "linear_bn_relu_dropout", "_bn_act_args", "_linear_bn_args",
         "_bn_relu_dropout_sync", "_BN_SYNC_STAGES", "BN_DROP_ALL")


def test_names_are_the_same_objects_in_both_modules():
    import mccnn_amd.MCConvModule as M
    import mccnn_amd.dense_glue as G
    for name in NAMES:
        assert getattr(M, name) is getattr(G, name), name
    assert G.bn_relu_dropout.__module__ == "mccnn_amd.dense_glue"
    assert M.BN_DROP_ALL == 1 << 32 and len(M._BN_SYNC_STAGES) == 4 and all(callable(f) for f in M._BN_SYNC_STAGES)
    # what dense_glue takes from MCConvModule is MCConvModule's: one error class, one workspace pool
    assert G._req is M._req and G._ws is M._ws and G._bf16_rows_aligned is M._bf16_rows_aligned


@pytest.mark.parametrize("first", ["dense_glue", "MCConvModule"])
def test_either_module_may_be_imported_first(first):
    code = ("import mccnn_amd.%s\n"
            "import mccnn_amd.MCConvModule as M, mccnn_amd.dense_glue as G\n"
            "assert all(getattr(M, n) is getattr(G, n) for n in %r)\n" % (first, NAMES))
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, timeout=120)


def test_native_wrappers_resolve_and_end_in_the_ops_checks():
    import mccnn_amd.MCConvModule as M
    from mccnn_amd import _lib, native
    lib = _lib.load()
    before = lib.mccnn_debug_launch_count()
    x, w, b = torch.zeros(6, 8), torch.zeros(8, 8), torch.zeros(8)
    g, be, mm, mv = torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8)
    for f in (native.bn_relu_drop, native.bn_relu_drop_sync, native.linear_bn_relu_drop):
        assert callable(f)
    with pytest.raises(M.InvalidArgumentError, match="bn_relu_dropout: x must be a CUDA tensor"):
        native.bn_relu_drop(x, g, be, mm, mv, True, keepProb=0.5, seed=1)
    with pytest.raises(M.InvalidArgumentError, match="bn_relu_dropout expects keepProb"):
        native.bn_relu_drop_sync(x, g, be, mm, mv, keepProb=1.5)
    with pytest.raises(M.InvalidArgumentError, match="linear_bn_relu_dropout: x must be a CUDA tensor"):
        native.linear_bn_relu_drop(x, w, b, g, be, mm, mv, True, keepProb=0.5, seed=1)
    with pytest.raises(M.InvalidArgumentError, match="linear_bn_relu_dropout expects a seed"):
        native.linear_bn_relu_drop(x, w, b, g, be, mm, mv, True, seed=-1)
    assert lib.mccnn_debug_launch_count() == before


def test_a_keep_probability_that_keeps_nothing_is_refused_behind_the_other_checks():
    """floor(keepProb * 2^32) == 0: refused, but only once everything else is in order -- a call wrong in two ways gets the
    earlier check's text."""
    import mccnn_amd.MCConvModule as M
    x, g = torch.zeros(6, 8), torch.ones(8)
    with pytest.raises(M.InvalidArgumentError, match="x must be a CUDA tensor"):
        M._bn_act_args(x, g, g, g, g, 1e-12, 0)
    with pytest.raises(M.InvalidArgumentError, match="x must be a CUDA tensor"):
        M._linear_bn_args(x, torch.zeros(8, 8), g, g, g, g, g, 1e-12, 0)
