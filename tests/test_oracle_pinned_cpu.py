"""The oracle against RECORDED outputs of the reference's own kernels -- no GPU, no reference library needed.

tests/golden/ref_<case>.npz hold what the reference's kernels (its tf_ops/*.cu, compiled with hipcc for gfx950 by
oracle/ref_build.py) gave on an MI355X for the smallest cases of tests/ref_cases.py, each op fed the oracle's outputs of
the preceding ops; `python tests/ref_runner.py --golden` on a GPU box rewrites them. The inputs are regenerated from
seeds. The comparisons are those of tests/test_gpu_reference.py (tests.ref_cases.compare): integer outputs bit for bit,
`indexs` and the Poisson samples up to the reference's atomic arrival order, floats at 1e-4. A change to the oracle
that departs from the reference -- a `<` turned `<=` on the neighbour radius, a floor turned round in the cell of a
point, two entries of the 27-cell table swapped -- fails here on any machine: the lattice cases decide thousands of
such comparisons exactly ON the boundary.
"""
import os

import numpy as np
import pytest

from tests import ref_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", rc.GOLDEN_CASES)
def test_oracle_matches_recorded_reference(oracle, name):
    case = rc.CASE_BY_NAME[name]
    with np.load(os.path.join(GOLDEN, "ref_%s.npz" % name)) as z:
        r = {k: z[k] for k in z.files}
    inp = rc.make_inputs(case)
    o = rc.run_ops(oracle, case, inp)
    assert set(rc.public(o)) == set(r), sorted(set(rc.public(o)) ^ set(r))
    errs = rc.compare(case, o, r, "oracle vs recorded reference", True)
    print(name, errs)


def test_golden_fixtures_are_small():
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("ref_"))
    for name in rc.GOLDEN_CASES:
        assert os.path.getsize(os.path.join(GOLDEN, "ref_%s.npz" % name)) <= largest, name


@pytest.mark.parametrize("name", ["lattice_abs", "lattice_scaleinv"])
def test_lattice_cases_decide_on_the_boundary(oracle, name):
    """At least a few hundred ordered pairs at EXACTLY the radius and a few hundred points EXACTLY on a cell face; the
    box is [0, 1]^3 bit for bit, so the scale-invariant radius and the cell size are exact too."""
    case = rc.CASE_BY_NAME[name]
    inp = rc.make_inputs(case)
    o = rc.run_ops(oracle, case, inp)
    assert np.all(o["aabbMin"] == 0.0) and np.all(o["aabbMax"] == 1.0)
    assert o["cellIndexs"].shape[1] == 16
    assert np.all(inp["pts"] * 64 == np.round(inp["pts"] * 64))
    assert len(np.unique(inp["pts"], axis=0)) < len(inp["pts"])       # duplicates
    on_face, at_radius = rc.boundary_census(case, inp, o)
    assert on_face >= 300 and at_radius >= 300, (on_face, at_radius)
    # the clamp at the upper face: points with a coordinate == max sit in the last cell, not one past it
    top = np.any(inp["pts"] == 1.0, axis=1)
    assert top.sum() >= 20 and o["keys"][top].max() < case["B"] * 16 ** 3


def test_binding_resolves_every_launcher_once():
    """Every launcher oracle/ref.py names is found in the built library exactly once under the parameter list the
    binding passes (computeAuxiliarBuffersSize twice, once per overload)."""
    from oracle import ref, ref_build
    if not ref_build.available():
        pytest.skip("oracle/_ref/libmccnn_ref.so is absent: built by oracle/ref_build.py where the reference sources are")
    found = ref.resolve(ref_build.LIB)
    assert set(found) == set(ref.LAUNCHERS)
    for key, syms in found.items():
        name, sig, _ = ref.LAUNCHERS[key]
        assert len(syms) == 1, "%s%s resolves to %r" % (name, ref.param_list(sig), syms)
    assert found["sort_aux"] != found["neigh_aux"]
    assert len({s[0] for s in found.values()}) == len(found)


def test_recipe_does_nothing_without_the_reference_sources(monkeypatch, tmp_path):
    from oracle import ref_build
    before = os.path.getmtime(ref_build.LIB) if ref_build.available() else None
    monkeypatch.setenv(ref_build.REF_ENV, str(tmp_path / "no_such_directory"))
    assert ref_build.build(force=True) is None
    assert (os.path.getmtime(ref_build.LIB) if ref_build.available() else None) == before
