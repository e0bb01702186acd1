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
and full storage, without sections and with one section equal to the context's material; and the matrix-free product
(k_element_product, all four instantiations: triangles or quadrilaterals in the plan, without and with sections), on which
prescribed displacements and support reactions are built.  Every element has nodes of its own, so the 3x3 or 4x4 blocks of
K that an element touches are its matrix, and the product with "dof a of local node i of every element = 1" is column (i, a)
of every element's matrix, exactly (truth.probe_element_matrices): both triangles of the matrix are read, so symmetry is a
measurement on that path.  femshell_reactions and the prescribed right-hand side are the same kernel with other arguments
and are held to the product's bits on the thin flat families.

One section equal to the context's material cannot tell a kernel that reads the context's constants from one that reads the
section's.  The "own" paths can: the families with more than one material (T3 and Q4: thickness 1e-5 to 0.1; T6: nu up to
0.4999999; T7: E = 1e-3 and 1e11) run as one mesh each, and six families as one mixed mesh, every element with a section of
its own material under a context whose material (truth.OWN_CONTEXT) is no element's, through k_element_matrices, both
assembly kernels in both storages, and the product.

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


def family_within_its_budget(monkeypatch, fam, path):
    reached = []
    worst = truth.device_family_errors(pkg, monkeypatch.setenv, FX, fam, path, reached=reached)
    print(report(fam, path, worst))
    if path[0] == truth.PRODUCT:  # every context of the family launched the instantiation this case is there for
        assert reached and set(reached) == {(fam[0] == "Q", bool(path[2]))}, reached
    assert not truth.check(FX, fam, worst, FACTORS.get(fam)), report(fam, path, worst)


@pytest.mark.parametrize("path", truth.PATHS, ids=truth.path_id)
@pytest.mark.parametrize("fam", truth.FAMILIES)
def test_family_within_its_error_budget(monkeypatch, fam, path):
    family_within_its_budget(monkeypatch, fam, path)


@pytest.mark.parametrize("path", truth.OWN_PATHS, ids=truth.path_id)
@pytest.mark.parametrize("fam", truth.OWN_FAMILIES)
def test_family_with_a_section_per_material_within_its_error_budget(monkeypatch, fam, path):
    """The whole family in one mesh, every element with a section of its own material, under a context whose material
    (truth.OWN_CONTEXT) is no element's: a kernel that reads the context's membrane constant, bending constant or nu where it
    should read the section's is wrong in every element.  On T3 and Q4 the thickness spans four decades inside one section
    table, and the membrane, bending and drilling entries are held each on their own scale."""
    assert len(truth.groups_of(FX, fam)) > 1 and len(truth.groups_of(FX, fam, own=True)) == 1
    family_within_its_budget(monkeypatch, fam, path)


MIXED = ("T1", "T4", "T5", "Q1", "Q3", "Q6")
MIXED_OWN = ("T3", "T4", "T6", "T7", "Q3", "Q4")


def mixed_mesh_within_budgets(monkeypatch, path, families, members, material):
    """`members` (family, element) in one mesh under a context of `material`, each element held to its family's bound (whole
    matrix, symmetry, translations); on an "own" path every element has a section of its own material."""
    tris = [m for m in members if m[0][0] == "T"]
    quads = [m for m in members if m[0][0] == "Q"]
    assert len(tris) >= 16 and len(quads) >= 16
    own = path[2] == "own"
    reached = []
    Kt, Kq = truth.device_matrices(pkg, monkeypatch.setenv, path, material,
                                   [FX[f + "_xyz"][e] for f, e in tris], [FX[f + "_xyz"][e] for f, e in quads],
                                   [truth.material_of(FX, f, e)[:3] for f, e in tris] if own else None,
                                   [truth.material_of(FX, f, e)[:3] for f, e in quads] if own else None, reached)
    if path[0] == truth.PRODUCT:
        assert reached == [(True, bool(path[2]))], reached
    worst = {fam: {m: 0.0 for m in ("whole", "symmetry", "translation")} for fam in families}
    for (fam, e), copies in zip(tris + quads, Kt + Kq):
        for K in copies:
            err = truth.element_errors(K, truth.truth_of(FX, fam, e))
            for m in worst[fam]:
                worst[fam][m] = max(worst[fam][m], err[m])
    bad = []
    for fam in families:
        print(fam, truth.path_id(path), worst[fam])
        for m, w in worst[fam].items():
            b = truth.bound(float(FX["%s_err_%s" % (fam, m)].max()), FACTORS.get(fam, {}).get(m, 4.0))
            if not w <= b:
                bad.append((fam, m, w, b))
    assert not bad, bad


@pytest.mark.parametrize("path", truth.PATHS, ids=truth.path_id)
def test_mixed_mesh_within_the_budgets_of_its_families(monkeypatch, path):
    """Triangles and quadrilaterals in one mesh: quadrilateral records change the record layout for the triangles too.  The
    elements of six families that have the default material, each held to its family's bound (whole matrix, symmetry,
    translations)."""
    members = [(fam, e) for fam in MIXED for e in range(truth.PER_FAMILY)
               if truth.material_of(FX, fam, e) == tuple(truth.DEFAULT_MATERIAL[:3]) + (3,)]
    mixed_mesh_within_budgets(monkeypatch, path, MIXED, members, truth.material_of(FX, "T1", 0))


@pytest.mark.parametrize("path", truth.OWN_PATHS, ids=truth.path_id)
def test_mixed_mesh_with_a_section_per_material_within_the_budgets_of_its_families(monkeypatch, path):
    """Triangles and quadrilaterals with sections in one mesh: the element's material travels in other words of the record than
    in a mesh of triangles (shell_element.hpp rec_put_section), and a quadrilateral takes its membrane and bending constants
    from there too.  The flags-3 elements of six families, nine materials in one table, under truth.OWN_CONTEXT."""
    members = [(fam, e) for fam in MIXED_OWN for e in range(truth.PER_FAMILY) if truth.material_of(FX, fam, e)[3] == 3]
    assert len({truth.material_of(FX, fam, e)[:3] for fam, e in members}) >= 8
    mixed_mesh_within_budgets(monkeypatch, path, MIXED_OWN, members, truth.OWN_CONTEXT + (3,))


@pytest.mark.parametrize("fam", ("T3", "Q4"))
def test_reactions_and_prescribed_rhs_are_the_element_product_bit_for_bit(fam):
    """femshell_reactions and the right-hand side of prescribed displacements are k_element_product with other arguments (loads
    subtracted; u_bar as x, the mask and the sign in the epilogue): on the thin flat families, for every probe vector of
    truth.probe_element_matrices, they give the bits of femshell_element_product, so its budget above is theirs."""
    nodes = truth.nodes_of(fam)
    for material, els in truth.groups_of(FX, fam).items():
        X = [FX[fam + "_xyz"][e] for e in els]
        reps = -(-truth.MIN_ELEMENTS // len(els))
        xyz, tri, quad = truth.isolated_mesh(X if nodes == 3 else None, X if nodes == 4 else None, reps)
        conn = list(tri) + list(quad)
        n = len(xyz)
        assert len(conn) >= truth.MIN_ELEMENTS
        nu, E, t, flags = material
        fs = pkg.FemShell(nu, E, t, flags=flags)
        fs.set_mesh(xyz, tri, quad)
        probes = [(i, a) for i in range(nodes) for a in range(6)]
        columns = {}
        for i, a in probes:
            e = truth.probe_vector(n, conn, i, a)
            col = columns[i, a] = fs.element_product(e).reshape(n, 6)
            assert np.abs(col).max() > 0.0
            np.testing.assert_array_equal(fs.reactions(e), col, err_msg="reactions, no loads, probe %d %d" % (i, a))
            # F = mask(0 - K_unc u_bar), u_bar = e on the dofs that are fixed: dof a of local node i of every element
            mask = np.zeros(n, np.uint8)
            mask[[c[i] for c in conn]] = 1 << a
            fs.set_dirichlet(mask)
            fs.set_prescribed(e)
            fs.assemble()
            F = fs.export_bsr()[3].reshape(n, 6)
            np.testing.assert_array_equal(F, np.where(e != 0.0, 0.0, -col), err_msg="prescribed rhs, probe %d %d" % (i, a))
            assert not F[e != 0.0].any() and not np.signbit(F[e != 0.0]).any()
        fs.set_prescribed(None)
        mask = np.zeros(n, np.uint8)
        mask[::3] = 0x15  # reactions are the same expression at fixed and at free dofs
        fs.set_dirichlet(mask)
        # loads of the size of the largest entry of every row of the element matrices
        loads = np.random.default_rng(13).normal(size=(n, 6)) * np.max([np.abs(c) for c in columns.values()], axis=0)
        fs.set_loads(loads)
        for i, a in probes:  # one correctly rounded subtraction per entry, at every dof
            np.testing.assert_array_equal(fs.reactions(truth.probe_vector(n, conn, i, a)), columns[i, a] - loads,
                                          err_msg="reactions under loads, probe %d %d" % (i, a))
        fs.close()
