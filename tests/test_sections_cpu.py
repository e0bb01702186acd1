"""Shell sections, CPU side: the reference the GPU tests of tests/test_gpu_sections.py compare against (the oracle's
assembly section by section, summed -- tests/helpers/sections.py) is itself pinned here, and every case a GPU solve test uses
is shown to be well enough conditioned that the reference sits decades inside the bounds used there."""
import numpy as np
import pytest

from tests.helpers import oracle, sections
from tests.helpers.product import ensure_built

pkg = ensure_built()


def test_the_binding_knows_the_new_entry_point():
    """femshell_set_sections is in the symbol list a library must export to be loaded (a stale one fails at load)"""
    binding = __import__("importlib").import_module("fem-shell_amd.binding")
    assert "femshell_set_sections" in binding.SYMBOLS
    assert hasattr(pkg.FemShell, "set_sections")
    assert hasattr(pkg.load_library(), "femshell_set_sections")


def test_split_sum_with_one_material_is_the_whole_mesh_assembly():
    m = sections.curved_patch(12, 9)
    mat = (0.3, 7.0e4, 0.05)
    sec = sections.strips_of(m.xyz, m.tri)
    r, c, v = sections.split_sum(m.xyz, m.tri, None, [mat] * 3, sec, None, m.dirichlet_mask())
    r0, c0, v0, _ = oracle.assemble(m.xyz, m.tri, m.quad, oracle.material(*mat), m.dirichlet_mask(), m.loads)
    np.testing.assert_array_equal(r, r0)
    np.testing.assert_array_equal(c, c0)
    assert np.abs(v - v0).max() <= 1e-11 * np.abs(v0).max()


@pytest.mark.parametrize("flags", [3, 0])
@pytest.mark.parametrize("case", ["strips", "mixed"])
def test_split_sum_is_the_sum_of_single_elements_with_their_own_material(case, flags):
    """oracle.element_tri3 / element_quad4 with the element's own material, scattered in Python, against the split sum
    without constraints: block by block"""
    cs = sections.three_strips(12, 9) if case == "strips" else sections.mixed_patch()
    r, c, v = sections.split_sum(cs.xyz, cs.tri, cs.quad, cs.sections, cs.tri_section, cs.quad_section, None, flags)
    r1, c1, v1 = sections.element_sum(cs, flags)
    np.testing.assert_array_equal(r, r1)
    np.testing.assert_array_equal(c, c1)
    assert np.abs(v - v1).max() <= 1e-11 * np.abs(v1).max()
    assert len(np.unique(np.r_[cs.tri_section, cs.quad_section])) == 3  # every strip is there


@pytest.mark.parametrize("case", ["ibeam", "strips"])
def test_the_solve_cases_are_well_conditioned(case):
    """K symmetric, the oracle's PCG converges and agrees with the refined direct solve, the plain direct solve does too:
    the reference alone is far inside the 1e-9 of the GPU solve tests"""
    cs = sections.ibeam() if case == "ibeam" else sections.three_strips()
    r, c, v, F = sections.reference(cs)
    K = oracle.to_scipy(r, c, v)
    assert abs(K - K.T).max() <= 1e-11 * abs(K).max()
    u_ref = oracle.refined_solve(r, c, v, F)
    u_cg, info = oracle.pcg(r, c, v, F, rtol=1e-13, max_it=20000)
    assert info["converged"] == 1
    print("%s: oracle PCG %d iterations" % (case, info["iterations"]))
    assert np.linalg.norm(u_cg - u_ref) <= 1e-11 * np.linalg.norm(u_ref)
    assert np.linalg.norm(oracle.direct_solve(r, c, v, F) - u_ref) <= 1e-11 * np.linalg.norm(u_ref)


def test_the_mesh_between_the_caps_is_what_its_name_says():
    """the fullest slice of that panel touches more elements than the pipelined kernel takes with sections and fewer than it
    takes without, and the plan lays it out for the pipelined kernel"""
    cs = sections.tapered_panel(**sections.BETWEEN_THE_CAPS)
    plan = pkg.build_plan(cs.xyz, cs.tri)
    most = int(np.diff(plan["slice_elem_ptr"]).max())
    assert plan["pipe"] == 1 and 134 < most <= 150, most
    plain = sections.tapered_panel(70, 45)
    plan = pkg.build_plan(plain.xyz, plain.tri)
    assert plan["pipe"] == 1 and int(np.diff(plan["slice_elem_ptr"]).max()) <= 134
