"""The derived element kernels against an extended-precision truth (tests/golden/derived_truth.npz, written by
tools/gen_golden_derived_truth.py; tests/helpers/derived_truth.py has the metrics): k_element_resultants (femshell_element_resultants),
k_geometric_coeff and k_geometric_product (femshell_geometric_product), k_element_loads (femshell_element_load_vector) and
k_lumped_mass (femshell_lumped_mass).

The older tests of these kernels compare with an FP64 numpy reference to 1e-12 of an absolute-sum scale, on well-shaped meshes of
unit size with one material.  FP64 delivers 3e-16 to 2e-14 there, so that bar accepts a kernel that is wrong at 1e-13 of its
result, and no sliver, no far-away quadrilateral, no nu = 0.4999999 and no thickness of 1e-5 ever reached them.  Here the
reference is the same numpy formulas in long double on the 13 families of tests/golden/element_truth.npz, in two displacement
states (random; a smooth field of strain 1e-4), and the bound is an error budget, as in tests/test_gpu_element_truth.py:

    device's worst error over a family  <=  max(4 x the FP64 reference's worst error over that family, 16 eps)

per family, state, metric and path (truth.bound has the reasoning for 4 and for 16 eps).  The reference's errors are in the
fixture, re-checked by tests/test_derived_truth_cpu.py; none of these numbers comes from the device.  Metrics: N, M (2-norm over
the six global components), the two von Mises values, g (Frobenius), the load shares and the masses (translational and rotational
each on their own scale) against the truth; and without any formula of the reference's: N ez = M ez = 0 with the binary128 normal,
exact zeros on the flat families where truth and reference have them, the defect under a rigid motion on T1 and Q1, and g 1 = 0.

Every element has nodes of its own, repeated to at least truth.MIN_ELEMENTS elements, and every copy is held to the bound.  Paths:
no sections (triangle families launch k_element_resultants<false, false>, quadrilateral families <true, false> with no triangle
in the plan), one section equal to the context's material, and "own" -- the families with more than one material as one mesh
each, every element with a section of its own material and density under a context whose material (truth.OWN_CONTEXT) is no
element's: a kernel that reads the context's t, nu or cp where it should read the section's is wrong in every element -- and the
two mixed meshes of tests/test_gpu_element_truth.py, where a triangle takes the 10-word coefficient row and the other record
layout.

What the first run found: on the far quadrilaterals Q3 the kernels were 1.4e-10 from the truth in M and 1.9e-10 in g, and on Q1
(an element of size 0.24 at distance 8) the von Mises values at 5.3 times the reference's error, because quad4_means and
quad4_coeff projected absolute coordinates on the frame and differenced the projections.  The reference did the same, so Q3 sat
inside a budget of 6e-10 that tested nothing.  k_element_resultants and k_geometric_coeff now subtract the element's first node
before the projection, the reference of this test does the same (rs.quad4_frame relative=True), and Q3 is held to 4e-15 to
7e-15 like every other family.

profiles/derived_truth_vs_long_double.txt has the ratios device error / reference error measured after that fix
(tools/derived_truth_report.py prints that table): the largest is 8.1 (g of Q5 in the smooth state, see FACTORS), the next 2.5
(g of Q6), no family over its bound.  The table was taken again when quad4_means moved onto the QUAD4 geometry it shares with
quad4_record (shell_element.hpp; no `#pragma clang fp` there): M, vm, plane and frame of the quadrilateral families moved in
their last digits, N and g did not, and the two largest ratios are the same.
"""
import pytest

from tests.helpers import derived_truth as dt, truth
from tests.helpers.product import ensure_built
from tests.test_gpu_element_truth import MIXED, MIXED_OWN

pytestmark = pytest.mark.gpu
pkg = ensure_built()
FX = dict(truth.load())
DX = dict(dt.load())

# Families and metrics whose factor is not 4.  (A family over its bound is a finding: the cause is looked for in
# element_resultants.hip, geometric_stiffness.hip, element_loads.hip or dynamics_kernels.hip and fixed there.  Only a cause
# inherent to any FP64 evaluation of the formula may raise the factor of that one family and metric, to twice the measured ratio
# and never above 16, with the reasoning written here.)
#
# Q5, g: measured 8.83e-15 against the reference's 1.09e-15 in the smooth state, ratio 8.1, factor 16 (twice the ratio is 16.1).
# The family's worst is element 0 in the smooth state, where the membrane force itself is a cancelled sum -- N_loc = (-2.9, -3.0,
# -5.9) on an absolute-sum scale of (38, 121, 18) -- and g cancels again: |g| is 1/82 of its absolute sum, so an FP64 evaluation
# owes it about 82 eps = 1.8e-14, and the reference's own 4.3e-16 on that element is a lucky draw, not a bound.  The same numpy
# formulas in FP64 on the same element, with the coordinates shifted by exact amounts (absolute; relative to node 2; relative to
# node 0), are off by 1.7e-14, 7.9e-15 and 4.3e-16 (tests/test_derived_truth_cpu.py asserts that spread): the device's 8.8e-15
# lies inside it.  No other metric of Q5 is over its bound of 4.
FACTORS = {"Q5": {"g": 16.0}}


def family_within_its_budget(fam, sectioned):
    reached = []
    worst = dt.device_family_worst(pkg, FX, DX, fam, sectioned, reached)
    print(dt.report(DX, fam, dt.path_id(sectioned), worst))
    assert reached and set(reached) == {(fam[0] == "Q", bool(sectioned))}, reached  # the instantiation this case is there for
    assert not dt.check(DX, fam, worst, FACTORS.get(fam)), dt.report(DX, fam, dt.path_id(sectioned), worst)


@pytest.mark.parametrize("sectioned", dt.PATHS, ids=dt.path_id)
@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_family_within_its_error_budget(fam, sectioned):
    family_within_its_budget(fam, sectioned)


@pytest.mark.parametrize("fam", truth.OWN_FAMILIES)
def test_family_with_a_section_per_material_within_its_error_budget(fam):
    """The whole family in one mesh, every element with a section of its own material and density, under a context whose material
    (truth.OWN_CONTEXT) is no element's.  On T3 and Q4 the thickness spans four decades inside one section table:
    k_element_resultants<*, true> takes t from sec_t while 1 / t and 6 / t^2 feed the von Mises values, and the rotational masses
    go with t^3."""
    assert len(truth.groups_of(FX, fam)) > 1 and len(truth.groups_of(FX, fam, own=True)) == 1
    family_within_its_budget(fam, "own")


def mixed_mesh_within_budgets(families, elements, sectioned, material):
    members = [(fam, e, False) for fam, e in elements]
    assert sum(m[0][0] == "T" for m in members) >= 16 and sum(m[0][0] == "Q" for m in members) >= 16
    reached = []
    got = dt.device_results(pkg, material, members, sectioned, FX, DX, reached)
    assert reached == [(True, bool(sectioned))]
    bad = []
    for fam in families:
        els = [e for f, e in elements if f == fam]
        worst = dt.family_worst(FX, DX, fam, [got[(fam, e, False)] for e in els], elements=els)
        print(dt.report(DX, fam, "mixed-" + dt.path_id(sectioned), worst, dt.MIXED_METRICS))
        bad += [(fam,) + b for b in dt.check(DX, fam, worst, FACTORS.get(fam), dt.MIXED_METRICS)]
    assert not bad, bad


@pytest.mark.parametrize("sectioned", dt.PATHS, ids=dt.path_id)
def test_mixed_mesh_within_the_budgets_of_its_families(sectioned):
    """Triangles and quadrilaterals in one mesh: the elements of six families that have the default material, each held to its
    family's bound in N, M, vm, g, load and mass (and to its exact zeros)"""
    elements = [(fam, e) for fam in MIXED for e in range(truth.PER_FAMILY)
                if truth.material_of(FX, fam, e) == tuple(truth.DEFAULT_MATERIAL[:3]) + (3,)]
    mixed_mesh_within_budgets(MIXED, elements, sectioned, truth.material_of(FX, "T1", 0))


def test_mixed_mesh_with_a_section_per_material_within_the_budgets_of_its_families():
    """Triangles and quadrilaterals with sections in one mesh: the flags-3 elements of six families, nine materials and densities
    in one table, under truth.OWN_CONTEXT"""
    elements = [(fam, e) for fam in MIXED_OWN for e in range(truth.PER_FAMILY) if truth.material_of(FX, fam, e)[3] == 3]
    assert len({truth.material_of(FX, fam, e)[:3] for fam, e in elements}) >= 8
    mixed_mesh_within_budgets(MIXED_OWN, elements, "own", truth.OWN_CONTEXT + (3,))
