"""Elastic supports on the CPU: the reference of tests/helpers/elastic_support.py (longdouble, from the definition of
include/femshell.h) held to the properties of the definition, and what a foundation does to a plate, on the oracle."""
import importlib
import os
import re

import numpy as np
import pytest

from tests.helpers import dynamics, elastic_support as es, meshes, oracle, prescribed as pr, sections
from tests.helpers.product import ROOT

LD = np.longdouble


def _cases():
    xyz, tri = pr.panel(lift=True)
    tk, _ = es.random_moduli(len(tri), 0)
    yield "lifted_panel", xyz, tri, None, tk, None
    xyz, tri, quad = meshes.mixed_petals(24)
    tk, qk = es.random_moduli(len(tri), len(quad))
    yield "mixed_petals24", xyz, tri, quad, tk, qk
    xyz, tri = pr.panel(lift=True)
    strip = sections.strips_of(xyz, tri)  # moduli that follow the three sections
    yield "three_sections", xyz, tri, None, np.array([[4e3, 1e2], [0.0, 5e2], [7e2, 7e2]])[strip], None


CASES = list(_cases())
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name,xyz,tri,quad,tk,qk", CASES, ids=IDS)
def test_the_table_sums_to_the_foundation_of_the_whole_shell(name, xyz, tri, quad, tk, qk):
    """sum_a T_a = sum_e A_e [kt I + (kn - kt) n n^T] and tr T_a = sum share (kn + 2 kt), to 1e-13 of the absolute terms; the
    float64 evaluation of the same helper lies within 1e-13 T_a of the longdouble one"""
    S, T = es.table(xyz, tri, quad, tk, qk, dtype=LD)
    total = np.zeros((3, 3), LD)
    absolute = np.zeros((3, 3), LD)
    trace = np.zeros(len(xyz), LD)
    for conn, k in ((tri, tk), (quad, qk)):
        if conn is None:
            continue
        area, G = es.element_tensors(xyz, conn, k)
        total += (area[:, None, None] * G).sum(axis=0)
        absolute += (area[:, None, None] * np.abs(G)).sum(axis=0)
        kk = np.asarray(k).astype(LD)
        for i in range(conn.shape[1]):
            np.add.at(trace, conn[:, i], area / LD(conn.shape[1]) * (kk[:, 0] + 2 * kk[:, 1]))
    got = es.blocks(S)[:, :3, :3].sum(axis=0)
    err = np.abs(got - total)
    print("table sums %-16s: max |sum T - total| / sum |terms| = %.2e" % (name, float((err / absolute).max())))
    assert (err <= 1e-13 * absolute).all()
    assert (np.abs(S[:, :3].sum(axis=1) - trace) <= 1e-13 * trace).all() and trace.max() > 0
    assert not S[:, 6:].any()
    S64, _ = es.table(xyz, tri, quad, tk, qk, work=np.float64)
    ratio = es.bound_ratio(S64, S.astype(np.float64), T, tol=1e-13)
    print("table sums %-16s: float64 against longdouble / (1e-13 T_a) = %.3e" % (name, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("name,xyz,tri,quad,tk,qk", CASES[:2], ids=IDS[:2])
def test_an_isotropic_foundation_is_the_translational_lumped_mass(name, xyz, tri, quad, tk, qk):
    """kn = kt = k: T_a = k (translational lumped mass) / (rho t) I, to 1e-13, against tests/helpers/dynamics.py"""
    k, rho, t = 1e4, 7.8e-3, 0.37
    S, _ = es.table(xyz, tri, quad, np.full((len(tri), 2), k), None if quad is None else np.full((len(quad), 2), k))
    mass = dynamics.lumped_mass(xyz, tri, quad, rho, t)
    want = k * mass[:, 0] / (rho * t)
    assert (want > 0).any()
    assert (np.abs(S[:, :3] - want[:, None]) <= 1e-13 * want[:, None]).all()
    assert (np.abs(S[:, 3:6]) <= 1e-13 * want[:, None]).all()


@pytest.mark.parametrize("name,xyz,tri,quad,tk,qk", CASES, ids=IDS)
def test_every_block_is_positive_semi_definite(name, xyz, tri, quad, tk, qk):
    S, _ = es.table(xyz, tri, quad, tk, qk, es.random_springs(len(xyz)))
    B = es.blocks(S)[:, :3, :3]
    low = np.linalg.eigvalsh(B)[:, 0]
    tr = np.trace(B, axis1=1, axis2=2)
    assert (low >= -1e-13 * tr).all()
    assert (S[:, 6:] >= 0).all()


@pytest.mark.parametrize("name,xyz,tri,quad,tk,qk", CASES[:2], ids=IDS[:2])
def test_a_free_shell_on_an_isotropic_foundation_translates_rigidly(name, xyz, tri, quad, tk, qk):
    """No Dirichlet dof, k = 1e4, loads k A_a d on the translations, d = (1, 2, 3) 1e-3: the oracle's K_unc + K_sup solved directly
    (LAPACK, dense) gives u = d and no rotation.  Measured when this was written: 9.9e-13 (lifted panel) and 3.5e-12 (mixed
    petals) of max |d| at condition numbers 5.8e4 and 4.3e4; the bound is 1e-11."""
    k, d = 1e4, np.array([1.0, 2.0, 3.0]) * 1e-3
    n = len(xyz)
    S, _ = es.table(xyz, tri, quad, np.full((len(tri), 2), k), None if quad is None else np.full((len(quad), 2), k))
    loads = np.zeros((n, 6))
    loads[:, :3] = S[:, :1] * d  # T_a = k A_a I
    K_unc, _ = pr.matrices(xyz, tri, quad, oracle.material(pr.NU, pr.E, pr.T), np.zeros(n, np.uint8))
    A = oracle.to_scipy(*es.add_to_bsr(K_unc, S)).toarray()
    u = np.linalg.solve(A, loads.ravel()).reshape(n, 6)
    err = max(np.abs(u[:, :3] - d).max(), np.abs(u[:, 3:]).max()) / np.abs(d).max()
    print("rigid translation %-16s: max |u - d| / max |d| = %.2e, condition %.1e" % (name, err, np.linalg.cond(A)))
    assert err <= 1e-11


def test_the_plate_on_a_winkler_foundation_converges_with_h_squared():
    """The regular 10 x 10 panel of tests/test_element_loads_cpu.py (E 1e7, nu 0.3, t 0.5, p 300, edges 0x7) with kn = 1e4, kt = 0:
    the centre deflection against Navier's series with the foundation term (0.0312896; the unsupported plate gives 0.106466) at
    n = 8, 16, 32.  Measured when this was written: relative errors -1.946e-2, -4.935e-3, -1.240e-3, ratios 3.94 and 3.98.  All
    errors negative, both ratios in [3.5, 4.5], the band of the pressure test."""
    from tests.helpers import element_loads as el
    E, nu, t, p, kn = 1e7, 0.3, 0.5, 300.0, 1e4
    D = E * t ** 3 / (12.0 * (1.0 - nu * nu))
    exact = es.navier_centre(10.0, D, p, kn)
    assert abs(exact - 0.0312896) <= 5e-7 and abs(es.navier_centre(10.0, D, p, 0.0) - 0.106466) <= 5e-6
    errs = []
    for n in (8, 16, 32):
        xyz, tri = pr.panel(nx=n, ny=n, lx=10.0, ly=10.0, jitter=0)
        mask = np.zeros(len(xyz), np.uint8)
        for axis, value in ((0, 0.0), (0, 10.0), (1, 0.0), (1, 10.0)):
            mask[pr.edge_nodes(xyz, axis, value)] = 0x7
        loads, _ = el.load_vector(xyz, tri, None, np.tile([p, 0.0, 0.0, 0.0], (len(tri), 1)), None)
        S, _ = es.table(xyz, tri, None, np.tile([kn, 0.0], (len(tri), 1)), None)
        _, K_c = pr.matrices(xyz, tri, None, oracle.material(nu, E, t), mask)
        rhs = np.where(pr.fixed_dofs(mask), 0.0, loads.ravel())
        u = oracle.refined_solve(*es.add_to_bsr(K_c, S, mask), rhs).reshape(-1, 6)
        centre = (n // 2) * (n + 1) + n // 2
        assert np.allclose(xyz[centre], [5.0, 5.0, 0.0])
        errs.append(u[centre, 2] / exact - 1.0)
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("plate on a foundation: relative errors %s, ratios %s" % (["%.3e" % e for e in errs], ["%.3f" % r for r in ratios]))
    assert all(e < 0 for e in errs)
    assert all(3.5 <= r <= 4.5 for r in ratios)


def test_header_and_binding_agree():
    binding = importlib.import_module("fem-shell_amd.binding")
    pkg = importlib.import_module("fem-shell_amd")
    for sym in ("femshell_set_foundation", "femshell_set_springs", "femshell_support_stiffness", "femshell_support_forces"):
        assert sym in binding.SYMBOLS
    header = open(os.path.join(ROOT, "include", "femshell.h")).read()
    assert int(re.search(r"FEMSHELL_KERNEL_ELASTIC_SUPPORT = (\d+)", header).group(1)) == binding.KERNEL_ELASTIC_SUPPORT == pkg.KERNEL_ELASTIC_SUPPORT == 18
    assert re.search(r"int femshell_set_foundation\(femshell_ctx \*ctx, const double \*tri_k[^;]*, *\n? *const double \*quad_k[^;]*\);", header)
    assert re.search(r"int femshell_set_springs\(femshell_ctx \*ctx, int32_t n, const int32_t \*node_ids, const double \*k6\);", header)
    assert re.search(r"int femshell_support_stiffness\(femshell_ctx \*ctx, double \*out[^;]*\);", header)
    assert re.search(r"int femshell_support_forces\(femshell_ctx \*ctx, const double \*u[^;]*, *\n? *double \*f6_out[^;]*\);", header)
    for method in ("set_foundation", "set_springs", "support_stiffness", "support_forces"):
        assert hasattr(binding.FemShell, method)
