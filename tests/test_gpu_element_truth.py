"""The device's element stiffness against a quad-precision truth, part by part (tests/golden/element_truth.npz, written
by tools/gen_golden_truth.py; tests/helpers/truth.py has the metrics).

Every other check of the element math compares two FP64 evaluations, by one norm of the whole matrix, to 1e-12.  On a thin
flat shell (t/h = 1e-3) the bending entries are 1e-6 of the membrane entries, so that bar accepts a bending block that is
wrong at 1e-6 of itself; and where the two evaluations drift apart (quadrilaterals far from the origin, slivers) it cannot
say which one is right.  Here the reference is the same formulas in binary128, and the bound is an error budget:

    device's worst error over a family  <=  max(4 x the FP64 oracle's worst error over that family, 16 eps)

per family, metric and device path (truth.bound has the reasoning for 4 and for 16 eps).  The oracle's errors are in the
fixture, re-checked by tests/test_element_truth_cpu.py; none of these numbers comes from the device.  Metrics: the whole
matrix (Frobenius); on flat elements in a coordinate plane the membrane, bending and drilling entries each on their own
scale, and exact zeros where the truth has zeros (a non-zero there is a spurious membrane-bending coupling); on the generic
families the defect of K under a rigid motion of the element, which needs no formula of the oracle's; symmetry and zero
force under the three translations everywhere.  Invariance under renumbering an element's nodes is NOT asserted: the
drilling penalty and the as-coded Y(2,1) depend on the frame's first edge.

Device paths: femshell_element_matrices (k_element_matrices), and the assembly kernels, whose lean record builders
(RecLean, RecLeanSec) and sectioned instantiations that entry point does not run: k_assemble and k_assemble_pipe, symmetric
and full storage, without sections and with one section equal to the context's material.  Every element has nodes of its
own, so the 3x3 or 4x4 blocks of K that an element touches are its matrix.

profiles/element_truth_vs_quad.txt has the ratios device error / oracle error measured when this test was written
(tools/element_truth_report.py prints that table): the largest is 2.5 (membrane entries of T2), no family is over its bound.
"""
import numpy as np
import pytest

from tests.helpers import truth
from tests.helpers.product import ensure_built

pytestmark = pytest.mark.gpu
pkg = ensure_built()
FX = dict(truth.load())

# Families whose factor is not 4: none.  (A family over its bound is a finding: the cause is looked for in shell_element.hpp /
# assemble_kernel.hpp and fixed there.  Only a cause inherent to any FP64 evaluation of the formula may raise the factor of
# that one family, to twice the measured ratio and never above 16, with the reasoning written here.)
FACTORS = {}


def report(fam, path, worst):
    return "%s %s: " % (fam, truth.path_id(path)) + ", ".join(
        "%s %.2e (oracle %.2e)" % (m, worst[m], FX["%s_err_%s" % (fam, m)].max()) for m in truth.metrics_of(fam))


@pytest.mark.parametrize("path", truth.PATHS, ids=truth.path_id)
@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_family_within_its_error_budget(monkeypatch, fam, path):
    worst = truth.device_family_errors(pkg, monkeypatch.setenv, FX, fam, path)
    print(report(fam, path, worst))
    assert not truth.check(FX, fam, worst, FACTORS.get(fam)), report(fam, path, worst)


MIXED = ("T1", "T4", "T5", "Q1", "Q3", "Q6")


@pytest.mark.parametrize("path", truth.PATHS, ids=truth.path_id)
def test_mixed_mesh_within_the_budgets_of_its_families(monkeypatch, path):
    """Triangles and quadrilaterals in one mesh: quadrilateral records change the record layout for the triangles too.  The
    elements of six families that have the default material, each held to its family's bound (whole matrix, symmetry,
    translations)."""
    members = [(fam, e) for fam in MIXED for e in range(truth.PER_FAMILY)
               if truth.material_of(FX, fam, e) == tuple(truth.DEFAULT_MATERIAL[:3]) + (3,)]
    tris = [m for m in members if m[0][0] == "T"]
    quads = [m for m in members if m[0][0] == "Q"]
    assert len(tris) >= 16 and len(quads) >= 16
    Kt, Kq = truth.device_matrices(pkg, monkeypatch.setenv, path, truth.material_of(FX, "T1", 0),
                                   [FX[f + "_xyz"][e] for f, e in tris], [FX[f + "_xyz"][e] for f, e in quads])
    worst = {fam: {m: 0.0 for m in ("whole", "symmetry", "translation")} for fam in MIXED}
    for (fam, e), copies in zip(tris + quads, Kt + Kq):
        for K in copies:
            err = truth.element_errors(K, truth.truth_of(FX, fam, e))
            for m in worst[fam]:
                worst[fam][m] = max(worst[fam][m], err[m])
    bad = []
    for fam in MIXED:
        print(fam, truth.path_id(path), worst[fam])
        for m, w in worst[fam].items():
            b = truth.bound(float(FX["%s_err_%s" % (fam, m)].max()), FACTORS.get(fam, {}).get(m, 4.0))
            if not w <= b:
                bad.append((fam, m, w, b))
    assert not bad, bad
