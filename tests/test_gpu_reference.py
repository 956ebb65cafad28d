"""The oracle and the HIP ops against the REFERENCE's own kernels, run on the same GPU.

oracle/ref_build.py compiles the reference's six tf_ops/*.cu files (kernels and plain-pointer host launchers) with
hipcc for gfx950 -- not with nvcc -- into oracle/_ref/libmccnn_ref.so; oracle/ref.py calls the launchers in the
sequences of the reference's op wrappers. tests/ref_runner.py runs every case of tests/ref_cases.py through it ONCE, in a
child process of its own (a fault in code that has never run on this GPU must not take pytest along), and this module
compares, op by op on identical inputs (every op reads the ORACLE's outputs of the preceding ops):

    oracle vs reference   pins the oracle
    HIP    vs reference   pins the product directly
    HIP    vs oracle      as elsewhere in the suite, on the same feed

Bit for bit: aabbMin / aabbMax, keys, sort step 2 (points, batch ids, features, cell table), its gradient routing,
sort_features(_back), startIndexs, packedNeighs row by row AS WRITTEN, transform_indexs, get_sampled_features and its
gradient. Up to the reference's atomic arrival order: `indexs` (a permutation, keys[indexs] non-decreasing, the same
positions per cell) and the Poisson samples (same count and same index set per cloud; points and batch ids compared
after sorting by index). At RTOL = 1e-4, norm-wise and per element (tests.helpers.assert_float_close): compute_pdf,
spatial_conv and its seven gradients; the bf16-row layer's HIP rows within one bf16 step, as in test_gpu_configs.py.
No element of any integer output is exempt.

The module skips only when oracle/_ref/libmccnn_ref.so is absent. If the child fails, every test here fails and the
child is not started again.

MEASURED on an MI355X: see MEASURED below.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ref_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "oracle", "_ref", "libmccnn_ref.so")

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not os.path.exists(LIB), reason="oracle/_ref/libmccnn_ref.so is absent: the reference "
                                 "library is built by oracle/ref_build.py where the reference sources are")]

#: seconds for the child: ~1 s of reference kernels and up to ~35 s of CPU oracle per case (dense_blob), 25 cases,
#: plus start-up; ten times the time measured for the whole list
RUNNER_TIMEOUT = 1200

MEASURED = """
Reference compiled with hipcc for gfx950 (contraction at the compiler's default, as with nvcc), 25 cases, 51 tests
passed, 0 skipped, no integer element excluded, no seed replaced. Worst max|diff| / max|ref| per output over all cases
(the reference's float atomics make its own figures move in the last digit from run to run):

    output     oracle vs reference   HIP vs reference   HIP vs oracle
    pdfs       0 (bit for bit)       0 (mode 0)         0
    out        9.2e-7                7.6e-7             8.8e-7
    featGrad   1.2e-6                9.8e-7             1.4e-6
    dw1        1.2e-5                1.2e-5             4.2e-7
    db1        9.9e-6                9.7e-6             2.5e-7
    dw2        7.2e-6                7.1e-6             3.9e-7
    db2        1.3e-5                1.3e-5             4.1e-7
    dw3        9.9e-6                9.9e-6             2.7e-7
    db3        1.8e-5                1.8e-5             4.1e-7

Of these, the two depth-wise layers whose width is no multiple of 8 (conv_dw12_padded, conv_dw4_noavg_abs: the reference's
op wrapper refuses them, spatial_conv.cc:292-296, its kernels -- called here through their launchers -- compute them; on
the HIP side the scalar instantiations of the edge-streaming kernels):

    out        6.7e-7                5.4e-7             4.7e-7
    featGrad   2.1e-7                3.2e-7             2.4e-7
    dw1        1.2e-5                1.2e-5             2.2e-7
    db1        9.9e-6                9.7e-6             1.9e-7
    dw2        6.6e-6                6.5e-6             3.9e-7
    db2        5.4e-6                5.4e-6             2.5e-7
    dw3        8.9e-6                8.9e-6             2.3e-7
    db3        8.1e-6                7.9e-6             2.2e-7

(the oracle itself against float64 autograd at these widths: tests/test_oracle_depthwise_cpu.py, worst 2.9e-7.)

The parameter gradients of the reference are ~1e-5 from both other sides and those agree to 4e-7: the distance is the
reference's own summation (one float atomicAdd per edge and neuron into a single accumulator, ~1e5 terms), not a
ReLU' decision taken differently. bf16-row layer (HIP rows against the f32 rows of the reference, rounded): out and
featGrad equal or one bf16 step apart (worst 1.5e-4 / 2.1e-4 of max|ref|, the step being 2^-8 of the element); its
parameter gradients 1.4e-5.
"""


class HipOps:
    """The product's ops (mccnn_amd.MCConvModule, i.e. the HIP kernels through the C-ABI) behind the oracle's NumPy
    surface, so that run_ops can feed them the oracle's outputs."""
    IS_HIP = True

    def __init__(self, mc):
        import torch
        self.mc, self.torch = mc, torch

    def _w(self, a, dtype=None):
        a = np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)
        return self.torch.from_numpy(a).cuda()

    @staticmethod
    def _u(t):
        return t.detach().float().cpu().numpy() if t.is_floating_point() else t.detach().cpu().numpy()

    def compute_aabb(self, P, Bi, B, sI):
        return tuple(self._u(t) for t in self.mc.compute_aabb(self._w(P), self._w(Bi), B, sI))

    def sort_points_step1(self, P, Bi, mn, mx, B, cell, sI):
        return tuple(self._u(t) for t in self.mc.sort_points_step1(self._w(P), self._w(Bi), self._w(mn), self._w(mx), B, cell, sI))

    def sort_points_step2(self, P, Bi, F, keys, idx, mn, mx, B, cell, sI):
        return tuple(self._u(t) for t in self.mc.sort_points_step2(self._w(P), self._w(Bi), self._w(F), self._w(keys),
                                                                  self._w(idx), self._w(mn), self._w(mx), B, cell, sI))

    def sort_points_step2_grad(self, idx, gP, gF):
        # the op's own backward: a one-cell grid is enough, the routing depends on indexs alone
        n = len(idx)
        P = self._w(np.zeros((n, 3), np.float32)).requires_grad_(True)
        F = self._w(np.zeros_like(gF)).requires_grad_(True)
        one = np.ones((1, 3), np.float32)
        sP, _, sF, _ = self.mc.sort_points_step2(P, self._w(np.zeros((n, 1), np.int32)), F, self._w(np.zeros(n, np.int32)),
                                                 self._w(idx), self._w(0 * one), self._w(one), 1, 1.0, True)
        a, b = self.torch.autograd.grad([sP, sF], [P, F], [self._w(gP), self._w(gF)])
        return self._u(a), self._u(b)

    def sort_features_back(self, F, idx):
        return self._u(self.mc.sort_features_back(self._w(F), self._w(idx)))

    def sort_features(self, F, idx):
        return self._u(self.mc.sort_features(self._w(F), self._w(idx)))

    def find_neighbors(self, C_, Cb, sP, cells, mn, mx, radius, B, sI):
        return tuple(self._u(t) for t in self.mc.find_neighbors(self._w(C_), self._w(Cb), self._w(sP), self._w(cells),
                                                               self._w(mn), self._w(mx), radius, B, sI))

    def compute_pdf(self, sP, sB, mn, mx, start, packed, window, radius, B, sI, mode=0):
        return self._u(self.mc.compute_pdf(self._w(sP), self._w(sB), self._w(mn), self._w(mx), self._w(start),
                                           self._w(packed), window, radius, B, sI, mode=mode))

    def poisson_sampling(self, P, Bi, cells, mn, mx, radius, B, sI):
        return tuple(self._u(t) for t in self.mc.poisson_sampling(self._w(P), self._w(Bi), self._w(cells), self._w(mn),
                                                                 self._w(mx), radius, B, sI))

    def transform_indexs(self, a, b):
        return self._u(self.mc.transform_indexs(self._w(a), self._w(b)))

    def get_sampled_features(self, si, F):
        return self._u(self.mc.get_sampled_features(self._w(si), self._w(F)))

    def get_sampled_features_grad(self, si, F, g):
        Ft = self._w(F).requires_grad_(True)
        out = self.mc.get_sampled_features(self._w(si), Ft)
        return self._u(self.torch.autograd.grad([out], [Ft], [self._w(g)])[0])

    def _conv(self, a, fout, combin, B, radius, sI, avg, bf16, nostate):
        sP, sF, sB, pdfs, C_, start, packed, mn, mx, w1, w2, w3, b1, b2, b3 = a
        tw = [self._w(v).requires_grad_(True) for v in (w1, w2, w3, b1, b2, b3)]
        F = self._w(sF)
        if bf16:
            F = F.to(self.torch.bfloat16)   # exact: make_inputs rounded the values already
        F.requires_grad_(True)
        self.mc.KEEP_CONV_STATE = not nostate
        try:
            out = self.mc.spatial_conv(self._w(sP), F, self._w(sB), self._w(pdfs), self._w(C_), self._w(start),
                                       self._w(packed), self._w(mn), self._w(mx), *tw, fout, combin, B, radius, sI, avg)
        except BaseException:
            self.mc.KEEP_CONV_STATE = True
            raise
        return out, F, tw

    def spatial_conv(self, *a_and_attrs, bf16=False, nostate=False):
        out, _, _ = self._conv(a_and_attrs[:15], *a_and_attrs[15:], bf16, nostate)
        self.mc.KEEP_CONV_STATE = True
        return self._u(out)

    def spatial_conv_grad(self, *a_and_attrs, bf16=False, nostate=False):
        a, og, attrs = a_and_attrs[:15], a_and_attrs[15], a_and_attrs[16:]
        try:
            out, F, tw = self._conv(a, *attrs, bf16, nostate)
            out.backward(self._w(og).to(out.dtype))
            self.torch.cuda.synchronize()
        finally:
            self.mc.KEEP_CONV_STATE = True
        w1, w2, w3, b1, b2, b3 = tw
        return tuple(self._u(t.grad) for t in (F, w1, b1, w2, b2, w3, b3))


@pytest.fixture(scope="session")
def reference_outputs(tmp_path_factory):
    """Starts tests/ref_runner.py ONCE, as a fresh child with its own time limit; any failure is remembered, and every
    dependent test then fails without the child being started again (pytest caches a session fixture's error)."""
    out = str(tmp_path_factory.mktemp("reference"))
    cmd = [sys.executable, os.path.join(ROOT, "tests", "ref_runner.py"), "--out", out]
    try:
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=RUNNER_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        pytest.fail("the reference child ran past %d s; its output so far:\n%s" % (RUNNER_TIMEOUT, (e.stdout or "")[-4000:]),
                    pytrace=False)
    print(p.stdout)
    if p.returncode != 0 or not os.path.exists(os.path.join(out, "runner_done.txt")):
        pytest.fail("the reference child ended with status %s; the last case its log names is where it stopped:\n%s"
                    % (p.returncode, p.stdout[-4000:]), pytrace=False)
    return out


_ORACLE_RUNS = {}


def _oracle_run(oracle, case):
    if case["name"] not in _ORACLE_RUNS:
        inp = rc.make_inputs(case)
        _ORACLE_RUNS[case["name"]] = (inp, rc.run_ops(oracle, case, inp))
    return _ORACLE_RUNS[case["name"]]


def _load(reference_outputs, case):
    with np.load(os.path.join(reference_outputs, case["name"] + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _report(case, pair, errs):
    print("REFERR %s" % json.dumps(dict(case=case["name"], pair=pair, errs=errs), sort_keys=True))


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_oracle_matches_reference(reference_outputs, oracle, case):
    inp, o = _oracle_run(oracle, case)
    r = _load(reference_outputs, case)
    _report(case, "oracle_vs_reference", rc.compare(case, o, r, "oracle vs reference", True))


@pytest.mark.parametrize("case", rc.CASES, ids=[c["name"] for c in rc.CASES])
def test_hip_matches_reference_and_oracle(reference_outputs, mc, oracle, case):
    inp, o = _oracle_run(oracle, case)
    r = _load(reference_outputs, case)
    g = rc.run_ops(HipOps(mc), case, inp, src=o)
    _report(case, "hip_vs_reference", rc.compare(case, g, r, "HIP vs reference", True, got_bf16_rows=True))
    _report(case, "hip_vs_oracle", rc.compare(case, g, o, "HIP vs oracle", False, got_bf16_rows=True))


def test_lattice_cases_decide_on_the_boundary(oracle):
    """The lattice clouds hold at least a few hundred pairs at EXACTLY the radius and points EXACTLY on cell faces."""
    for name in ("lattice_abs", "lattice_scaleinv"):
        case = rc.CASE_BY_NAME[name]
        inp, o = _oracle_run(oracle, case)
        on_face, at_radius = rc.boundary_census(case, inp, o)
        assert on_face >= 300 and at_radius >= 300, (name, on_face, at_radius)
