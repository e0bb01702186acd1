"""Pins the reference of the prescribed-displacement tests (tests/helpers/prescribed.py) on the CPU oracle alone: a membrane
patch test with its closed form, and a displacement-controlled cantilever against its force-controlled twin."""
import numpy as np
import pytest

from tests.helpers import oracle, prescribed as pr


def test_membrane_patch_test_reproduces_the_field_and_the_edge_force():
    eps = 1e-3
    xyz, tri, mask, ubar, exact = pr.membrane_patch(eps)
    assert len(xyz) == 48 and len(tri) == 70 and (mask == 0).sum() == 24
    ref = pr.Reference(xyz, tri, None, oracle.material(pr.NU, pr.E, pr.T), mask, None, ubar)
    err = np.abs(ref.u - exact).max() / np.abs(exact).max()
    print("patch test: max error %.2e of the field's maximum" % err)
    assert err <= 1e-12
    force = pr.E * eps * pr.T * pr.LY
    rx = ref.r[pr.edge_nodes(xyz, 0, pr.LX), 0].sum()
    ry = ref.r[pr.edge_nodes(xyz, 1, pr.LY), 1].sum()
    print("edge x = Lx: sum r_x / (E eps t Ly) - 1 = %.2e; edge y = Ly: sum r_y / that = %.2e" % (rx / force - 1.0, ry / force))
    assert abs(rx - force) <= 1e-12 * force
    assert abs(ry) <= 1e-12 * force
    # the free dofs are in equilibrium
    assert np.abs(ref.r.ravel()[~ref.fixed]).max() <= 1e-12 * np.abs(ref.r).max()


@pytest.mark.parametrize("thickness", [pr.T, 0.05])
def test_displacement_controlled_cantilever_agrees_with_its_force_controlled_twin(thickness):
    xyz, tri, mask, ubar, tip = pr.cantilever(0.01)
    mat = oracle.material(pr.NU, pr.E, thickness)
    ref = pr.Reference(xyz, tri, None, mat, mask, None, ubar)
    assert np.array_equal(ref.u[tip, 2], np.full(len(tip), 0.01))
    # the twin: the edge free, loaded with the reactions just obtained
    mask2 = mask.copy()
    mask2[tip] = 0
    loads = np.zeros((len(xyz), 6))
    loads[tip, 2] = ref.r[tip, 2]
    twin = pr.Reference(xyz, tri, None, mat, mask2, loads, None)
    err = np.linalg.norm(twin.u - ref.u) / np.linalg.norm(ref.u)
    print("t = %g: twin differs by %.2e" % (thickness, err))
    assert err <= 1e-10
