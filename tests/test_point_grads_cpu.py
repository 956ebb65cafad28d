"""Gradients with respect to positions, the parts that need no GPU: the float64 reference of tests/pointgrad_ref.py against
the CPU oracle's forward, torch.autograd.gradcheck of that reference, and the new C-ABI entries (declared, exported, bound,
no scratch)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import pointgrad_ref as ref
from tests.helpers import make_cloud, make_mlp, run_chain
from mccnn_amd.workloads import conv_nb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("mccnn_spatial_conv_bwd_points", "mccnn_spatial_conv_bwd_points_workspace_bytes",
               "mccnn_compute_pdf_bwd_points", "mccnn_compute_pdf_bwd_points_workspace_bytes", "mccnn_edge_grad_reduce")


def _chain(oracle, n_per, B, radius, scaleInv, fin, seed=3):
    pts, bids = make_cloud(n_per, B, seed, "clustered")
    feats = (2 * np.random.default_rng(seed).random((len(pts), fin)) - 1).astype(np.float32)
    return run_chain(oracle, lambda a: a, lambda a: a, pts, bids, feats, B, radius, scaleInv), pts


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("scaleInv", [True, False])
def test_reference_pdf_matches_the_oracle(oracle, scaleInv):
    r, _ = _chain(oracle, 300, 2, 0.15, scaleInv, 3)
    got = ref.compute_pdf(ref.t64(r["sortPts"]), r["sortBatchs"], ref.t64(r["aabbMin"]), ref.t64(r["aabbMax"]),
                          r["startIndexs"], r["packedNeighs"], 0.2, 0.15, scaleInv)
    assert _rel(got.numpy(), r["pdfs"].reshape(-1)) <= 1e-5


@pytest.mark.parametrize("scaleInv", [True, False])
@pytest.mark.parametrize("combin,fin,fout", [(True, 3, 8), (True, 1, 5), (False, 16, 16)])
@pytest.mark.parametrize("avg", [True, False])
def test_reference_conv_matches_the_oracle(oracle, scaleInv, combin, fin, fout, avg):
    r, pts = _chain(oracle, 300, 2, 0.15, scaleInv, fin)
    w = make_mlp(conv_nb(fin, fout, combin), 11)
    args = (r["sortPts"], r["sortFeatures"], r["sortBatchs"], r["pdfs"], pts, r["startIndexs"], r["packedNeighs"],
            r["aabbMin"], r["aabbMax"], w["w1"], w["w2"], w["w3"], w["b1"], w["b2"], w["b3"])
    want = oracle.spatial_conv(*args, fout, combin, 2, 0.15, scaleInv, avg)
    T = ref.t64
    got = ref.spatial_conv(T(r["sortPts"]), T(r["sortFeatures"]), r["sortBatchs"], T(r["pdfs"]), T(pts), r["startIndexs"],
                           r["packedNeighs"], T(r["aabbMin"]), T(r["aabbMax"]), T(w["w1"]), T(w["b1"]), T(w["w2"]),
                           T(w["b2"]), T(w["w3"]), T(w["b3"]), fout, combin, 2, 0.15, scaleInv, avg)
    assert _rel(got.numpy(), want) <= 1e-5


@pytest.mark.parametrize("combin,fin,fout", [(True, 2, 4), (False, 8, 8)])
def test_reference_gradcheck(oracle, combin, fin, fout):
    """The reference's own gradients (w.r.t. points, centres, PDFs and box) against finite differences, on ~64 points and
    a fixed neighbour list."""
    r, pts = _chain(oracle, 32, 2, 0.3, True, fin, seed=5)
    w = make_mlp(conv_nb(fin, fout, combin), 12)
    T = ref.t64
    sp = T(r["sortPts"]).requires_grad_(True)
    c = T(pts).requires_grad_(True)
    pd = T(r["pdfs"]).requires_grad_(True)
    mn = T(r["aabbMin"]).requires_grad_(True)
    mx = T(r["aabbMax"]).requires_grad_(True)
    f = T(r["sortFeatures"])
    ws = {k: T(v) for k, v in w.items()}

    def conv(sp, c, pd, mn, mx):
        return ref.spatial_conv(sp, f, r["sortBatchs"], pd, c, r["startIndexs"], r["packedNeighs"], mn, mx, ws["w1"],
                                ws["b1"], ws["w2"], ws["b2"], ws["w3"], ws["b3"], fout, combin, 2, 0.3, True, True)

    def pdf(sp, mn, mx):
        return ref.compute_pdf(sp, r["sortBatchs"], mn, mx, r["startIndexs"], r["packedNeighs"], 0.2, 0.3, True)

    assert torch.autograd.gradcheck(conv, (sp, c, pd, mn, mx), eps=1e-6, atol=1e-6, rtol=1e-4)
    assert torch.autograd.gradcheck(pdf, (sp, mn, mx), eps=1e-6, atol=1e-6, rtol=1e-4)


def _declared():
    txt = open(os.path.join(ROOT, "include", "mccnn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(mccnn_[a-z0-9_]+)\s*\(", txt))


@pytest.fixture(scope="module")
def lib_path():
    from mccnn_amd import build
    return build.build()


def test_position_gradient_entries_are_declared_exported_and_bound(lib_path):
    from mccnn_amd import _lib
    declared = _declared()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path], text=True)
    exported = set(re.findall(r" T (mccnn_[a-z0-9_]+)", out))
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert lib.mccnn_spatial_conv_bwd_points_workspace_bytes(100000, 4) >= 2 * 100000 * 4
    assert lib.mccnn_compute_pdf_bwd_points_workspace_bytes(100000, 4) >= 2 * 100000 * 4


def test_position_gradient_kernels_use_no_scratch(lib_path, tmp_path):
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no ROCm llvm tools")
    copy = os.path.join(str(tmp_path), os.path.basename(lib_path))
    shutil.copy(lib_path, copy)
    subprocess.run([objdump, "--offloading", copy], capture_output=True, text=True, cwd=str(tmp_path))
    cos = sorted(os.path.join(str(tmp_path), f) for f in os.listdir(str(tmp_path)) if f.endswith("gfx950"))
    assert cos, "no gfx950 code object extracted"
    meta = {}
    for co in cos:
        txt = subprocess.run([readelf, "--notes", co], capture_output=True, text=True).stdout
        for blk in txt.split("- .agpr_count")[1:] if "- .agpr_count" in txt else txt.split("  - .")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            scr = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if name and scr:
                meta[name.group(1)] = int(scr.group(1))
    for pat in ("conv_bwd_points", "pdf_bwd_points", "edge_grad_reduce", "batch_sum"):
        hits = {k: v for k, v in meta.items() if pat in k}
        assert hits, pat
        for k, v in hits.items():
            assert v == 0, "%s: %d bytes of scratch per lane" % (k, v)
