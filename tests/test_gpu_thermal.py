"""Thermal loads on the device (femshell_set_expansion, femshell_set_thermal, femshell_thermal_load_vector and their FemShell
methods) against tests/helpers/thermal.py, the long-double reference tests/test_thermal_cpu.py pins, and against closed-form
states: the loads in force are (nodal + S) + T in every consumer, the free thermal state carries no stress and needs no reaction,
the clamped one carries -N_T and -M_T, and the geometric stiffness and the buckling factors are those of the equivalent
prescribed contraction.  Device values are held to 1e-12 of the absolute-sum scale of what they are sums of."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import buckling as bk, element_loads as el, oracle, prescribed as pr, resultants as rs, thermal as th
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

TINY = 1e-12
ALPHA = 1.2e-5
SEC_ALPHA = [1.1e-5, 2.3e-5, 0.7e-5]  # for the three sections of "panel_three_sections"


def _counts(tri, quad):
    return (0 if tri is None else len(tri)), (0 if quad is None else len(quad))


def _context(xyz, tri, quad, sec=None, material=(rs.NU, rs.E, rs.T)):
    fs = pkg.FemShell(*material)
    fs.set_mesh(xyz, tri, quad)
    if sec is not None:
        fs.set_sections(sec[0], sec[1], sec[2])
    return fs


def _expand(fs, sec):
    """alpha for the whole shell, or one per section where the mesh has sections"""
    if sec is None:
        fs.set_expansion(ALPHA)
        return None
    fs.set_expansion(0.0, SEC_ALPHA)
    return SEC_ALPHA


def _mask(n):
    mask = np.zeros(n, np.uint8)
    mask[::3] = 0x15
    mask[0] = 0x3F
    return mask


def _expected_F(mask, loads):
    return np.where(pr.fixed_dofs(mask), 0.0, np.asarray(loads, dtype=np.float64).ravel())


# ------------------------------------------------------------------ 1. device against reference

@pytest.mark.parametrize("name", list(rs.device_meshes()))
def test_load_vector_matches_the_reference(name, monkeypatch):
    """Seeded random (Tm, Tg) per element, alpha per section where there are sections: |T - T_ref| <= 1e-12 scale, entry by entry
    on all six components, exactly zero where the scale is.  Two calls give the same bits, one kind alone leaves the other cold,
    a Dirichlet set does not show, clearing returns zeros."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nt, nq = _counts(tri, quad)
    fs = _context(xyz, tri, quad, sec)
    assert not fs.thermal_load_vector().any()  # none set yet
    sa = _expand(fs, sec)
    assert not fs.thermal_load_vector().any()
    tt, qt = th.random_temps(nt, nq)
    fs.set_thermal(tt, qt)
    Tv = fs.thermal_load_vector()
    assert Tv.shape == (len(xyz), 6)
    T_ref, scale = th.load_vector(xyz, tri, quad, tt, qt, ALPHA, sec=sec, sec_alpha=sa)
    ratio = th.bound_ratio(Tv, T_ref, scale)
    print("thermal_vs_reference %-28s elements %5d  max |T - T_ref| / (1e-12 scale) = %.3e" % (name, nt + nq, ratio))
    assert ratio <= 1.0
    assert np.abs(Tv[:, :3]).max() > 0.0 and np.abs(Tv[:, 3:]).max() > 0.0  # the rotational rows are filled
    assert np.array_equal(Tv, fs.thermal_load_vector())
    fs.set_dirichlet(_mask(len(xyz)))
    assert np.array_equal(Tv, fs.thermal_load_vector())
    if nt and nq:  # one kind alone
        fs.set_thermal(tt, None)
        assert th.bound_ratio(fs.thermal_load_vector(), th.load_vector(xyz, tri, quad, tt, None, ALPHA, sec=sec, sec_alpha=sa)[0], scale) <= 1.0
        fs.set_thermal(None, qt)
        assert th.bound_ratio(fs.thermal_load_vector(), th.load_vector(xyz, tri, quad, None, qt, ALPHA, sec=sec, sec_alpha=sa)[0], scale) <= 1.0
    fs.set_thermal(None, None)
    assert not fs.thermal_load_vector().any()
    fs.set_thermal(tt, qt)
    assert np.array_equal(Tv, fs.thermal_load_vector())
    fs.close()


def test_a_uniform_alpha_serves_every_section():
    """n_sections == 0 on a context with sections: alpha for every element, each with its own E, nu, t"""
    xyz, tri, quad, sec, _ = rs.device_meshes()["panel_three_sections"]()
    fs = _context(xyz, tri, quad, sec)
    fs.set_expansion(ALPHA)
    tt, _ = th.random_temps(len(tri), 0, seed=8)
    fs.set_thermal(tt)
    T_ref, scale = th.load_vector(xyz, tri, None, tt, None, ALPHA, sec=sec)
    assert th.bound_ratio(fs.thermal_load_vector(), T_ref, scale) <= 1.0
    fs.set_expansion(0.0, SEC_ALPHA)  # a new alpha while temperatures are in force: the loads follow
    T_ref, scale = th.load_vector(xyz, tri, None, tt, None, ALPHA, sec=sec, sec_alpha=SEC_ALPHA)
    assert th.bound_ratio(fs.thermal_load_vector(), T_ref, scale) <= 1.0
    fs.close()


def test_wrong_lengths_are_refused_by_the_binding():
    xyz, tri, quad = rs.device_meshes()["mixed_petals24"]()[:3]
    fs = _context(xyz, tri, quad)
    fs.set_expansion(ALPHA)
    with pytest.raises(ValueError):
        fs.set_thermal(np.zeros((len(tri) + 1, 2)), None)
    with pytest.raises(ValueError):
        fs.set_thermal(None, np.zeros((len(quad) - 1, 2)))
    fs.close()


def test_interior_rows_cancel_under_a_uniform_temperature():
    """flat uniform panel, one section, uniform Tm: the force rows of T at interior nodes are zero to the bound (the outward
    pushes of the elements round a node close to a polygon); the boundary rows are not"""
    xyz, tri = th.isosceles_panel(nx=9, ny=7)
    fs = _context(xyz, tri, None)
    fs.set_expansion(ALPHA)
    temps = np.tile([55.0, 0.0], (len(tri), 1))
    fs.set_thermal(temps)
    Tv = fs.thermal_load_vector()
    _, scale = th.load_vector(xyz, tri, None, temps, None, ALPHA)
    lx, ly = xyz[:, 0].max(), xyz[:, 1].max()
    inner = (xyz[:, 0] > 1e-9) & (xyz[:, 0] < lx - 1e-9) & (xyz[:, 1] > 1e-9) & (xyz[:, 1] < ly - 1e-9)
    assert inner.sum() == 8 * 6
    ratio = th.bound_ratio(Tv[inner, :3], np.zeros((inner.sum(), 3)), scale[inner, :3])
    print("interior cancellation: max |T_force| / (1e-12 scale) = %.3e" % ratio)
    assert ratio <= 1.0
    assert not Tv[:, 3:].any()  # no gradient: the rotational rows are exactly zero
    assert (np.abs(Tv[~inner, :3]).max(axis=1) > 1e-3 * scale[~inner, :3].max(axis=1)).all()
    fs.close()


# ------------------------------------------------------------------ 2. the invariant: loads in force = (nodal + S) + T

@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24", "delaunay600_rcm", "panel_three_sections"])
def test_right_hand_side_is_nodal_plus_element_loads_plus_thermal(name, monkeypatch):
    """F at the free dofs is fl(fl(L + S) + T) with S and T as the two load vectors return them, zero at the fixed ones: with and
    without element loads, in every order of the three calls; a second set replaces the first, clearing leaves fl(L + S), and F
    is then bitwise that of a context that never called the new functions."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = len(xyz)
    nt, nq = _counts(tri, quad)
    mask = _mask(n)
    rng = np.random.default_rng(23)
    L1, L2 = rng.uniform(-50.0, 50.0, (n, 6)), rng.uniform(-50.0, 50.0, (n, 6))
    loads = el.random_loads(nt, nq, seed=3)
    a, b = th.random_temps(nt, nq, seed=3), th.random_temps(nt, nq, seed=4)

    def F_of(fs):
        return fs.export_bsr()[3]

    old = _context(xyz, tri, quad, sec)  # never calls the new functions
    old.set_dirichlet(mask)
    old.set_loads(L2)
    old.set_element_loads(*loads)
    old.assemble()
    for order in ("nodal_first", "thermal_first", "element_loads_last"):
        fs = _context(xyz, tri, quad, sec)
        fs.set_dirichlet(mask)
        _expand(fs, sec)
        if order == "nodal_first":
            fs.set_loads(L1)
            fs.set_thermal(*a)
        else:
            fs.set_thermal(*a)
            fs.set_loads(L1)
        fs.assemble()  # F by the assembly kernel
        Ta = fs.thermal_load_vector()
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L1 + Ta), err_msg=order)  # no element loads: S = 0
        fs.set_element_loads(*loads)  # F by k_rhs alone from here on
        S = fs.element_load_vector()
        np.testing.assert_array_equal(fs.thermal_load_vector(), Ta)
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, (L1 + S) + Ta), err_msg=order)
        fs.set_thermal(*b)
        Tb = fs.thermal_load_vector()
        assert not np.array_equal(Ta, Tb)
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, (L1 + S) + Tb), err_msg=order)
        fs.set_loads(L2)
        np.testing.assert_array_equal(fs.thermal_load_vector(), Tb)
        np.testing.assert_array_equal(fs.element_load_vector(), S)
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, (L2 + S) + Tb), err_msg=order)
        if order == "element_loads_last":  # the element loads leave first: nodal + T
            fs.set_element_loads(None, None)
            np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L2 + Tb), err_msg=order)
            fs.set_element_loads(*loads)
            np.testing.assert_array_equal(F_of(fs), _expected_F(mask, (L2 + S) + Tb), err_msg=order)
        fs.set_thermal(None, None)
        assert not fs.thermal_load_vector().any()
        np.testing.assert_array_equal(F_of(fs), _expected_F(mask, L2 + S), err_msg=order)
        np.testing.assert_array_equal(F_of(fs), F_of(old), err_msg=order)
        fs.assemble()
        for x, y in zip(fs.export_bsr(), old.export_bsr()):
            np.testing.assert_array_equal(x, y, err_msg=order)
        fs.close()
    old.close()


def test_prescribed_values_with_thermal_loads():
    """F = mask((nodal + S) + T - K_unc u_bar): the right-hand side, the solution and the reactions of a context that was given the
    same sum through set_loads"""
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    tip = pr.edge_nodes(xyz, 0, pr.LX)
    mask[tip] = 0x04
    ubar = np.zeros((n, 6))
    ubar[tip, 2] = 0.01
    L = np.random.default_rng(5).uniform(-1.0, 1.0, (n, 6))
    tl, _ = el.random_loads(len(tri), 0, seed=9)
    tt, _ = th.random_temps(len(tri), 0, seed=9)
    out = []
    for _ in range(2):
        fs = _context(xyz, tri, None)
        fs.set_dirichlet(mask)
        fs.set_preconditioner("jacobi")
        fs.set_prescribed(ubar)
        out.append(fs)
    fa, fb = out
    fa.set_loads(L)
    fa.set_element_loads(tl)
    fa.set_expansion(ALPHA)
    fa.set_thermal(tt)
    fb.set_loads((L + fa.element_load_vector()) + fa.thermal_load_vector())
    ua, ia = fa.solve(rtol=1e-12, max_it=50000)
    ub, ib = fb.solve(rtol=1e-12, max_it=50000)
    assert ia["converged"] == 1 and ia["iterations"] == ib["iterations"]
    Fa = fa.export_bsr()[3]
    np.testing.assert_array_equal(Fa, fb.export_bsr()[3])
    assert not np.array_equal(Fa, _expected_F(mask, (L + fa.element_load_vector()) + fa.thermal_load_vector()))  # u_bar shows
    np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(fa.reactions(), fb.reactions())
    fa.close()
    fb.close()


# ------------------------------------------------------------------ 3. closed-form states

FREE = {"isosceles_triangles": lambda: th.isosceles_panel() + (None,), "rectangles": lambda: (th.rectangle_panel()[0], None, th.rectangle_panel()[1])}
TM, TG = 37.0, -11.0


@pytest.mark.parametrize("kind", list(FREE))
def test_the_free_state_needs_no_reaction_and_carries_no_stress(kind):
    """u_free passed explicitly, zero nodal loads: femshell_reactions is zero at ALL nodes to 1e-12 of sum |K| |u| + scale of T, and
    femshell_element_resultants gives N, M and both von Mises values zero to 1e-12 of their scale (tests/test_thermal_cpu.py
    shows that the operators of these two meshes reproduce the free strains)"""
    xyz, tri, quad = FREE[kind]()
    nt, nq = _counts(tri, quad)
    fs = _context(xyz, tri, quad)
    fs.set_expansion(ALPHA)
    tt = np.tile([TM, TG], (nt, 1)) if nt else None
    qt = np.tile([TM, TG], (nq, 1)) if nq else None
    fs.set_thermal(tt, qt)
    u = th.free_state(xyz, ALPHA, rs.T, TM, TG, x0=(0.7, 0.3))
    r = fs.reactions(u)
    K_unc, _ = pr.matrices(xyz, tri, quad, oracle.material(rs.NU, rs.E, rs.T), np.zeros(len(xyz), np.uint8))
    _, t_scale = th.load_vector(xyz, tri, quad, tt, qt, ALPHA)
    scale = pr.row_scale(K_unc, u)[:, None] + t_scale
    ratio = float((np.abs(r) / (TINY * scale)).max())
    print("free state %-20s reactions: max |r| / (1e-12 (sum |K||u| + |T|)) = %.3e" % (kind, ratio))
    assert ratio <= 1.0
    assert np.abs(fs.thermal_load_vector()).max() > 1e6 * np.abs(r).max()  # the two parts are not small: they cancel
    res = fs.element_resultants(u)
    _, res_scale = th.mesh_resultants(xyz, tri, quad, u, tt, qt, ALPHA)
    ratio = th.bound_ratio(res, np.zeros_like(res), res_scale)
    print("free state %-20s resultants: max |N, M, vm| / (1e-12 scale) = %.3e" % (kind, ratio))
    assert ratio <= 1.0
    fs.set_thermal(None, None)  # without temperatures the same field is strained
    cold = fs.element_resultants(u)
    assert np.abs(cold[:, :12]).max() > 1e6 * np.abs(res[:, :12]).max()
    fs.close()


@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24", "coil300", "panel_three_sections", "delaunay600_rcm"])
def test_the_clamped_state_carries_the_thermal_forces(name, monkeypatch):
    """u = 0 passed explicitly: N is -N_T on the two in-plane diagonal components in the element frame, rotated to global axes, M is
    -M_T in the same way, sigma_top/bot = -(E alpha / (1 - nu)) (Tm +- Tg / 2) and the von Mises values their magnitudes -- the
    closed form, and the long-double restatement with it; with sections too.  A random u on top: the restatement alone."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nt, nq = _counts(tri, quad)
    fs = _context(xyz, tri, quad, sec)
    sa = _expand(fs, sec)
    tt, qt = th.random_temps(nt, nq, seed=12)
    fs.set_thermal(tt, qt)
    zero = np.zeros((len(xyz), 6))
    res = fs.element_resultants(zero)
    ref, scale = th.mesh_resultants(xyz, tri, quad, zero, tt, qt, ALPHA, sec=sec, sec_alpha=sa)
    closed = []
    for conn, temp, which in th._kinds(tri, quad, tt, qt):
        for e, c in enumerate(conn):
            m = th.material_of(e, which, rs.NU, rs.E, rs.T, ALPHA, sec, sa)
            closed.append(th.clamped_closed_form(xyz[c], m[0], m[1], m[2], m[3], temp[e, 0], temp[e, 1]))
    closed = np.array(closed)
    r_closed, r_ref = th.bound_ratio(res, closed, scale), th.bound_ratio(res, ref, scale)
    print("clamped state %-24s max |res - closed form| / (1e-12 scale) = %.3e, against the restatement %.3e" % (name, r_closed, r_ref))
    assert r_closed <= 1.0 and r_ref <= 1.0
    assert np.abs(res[:, :6]).max() > 0.0 and np.abs(res[:, 6:12]).max() > 0.0 and res[:, 12:].min() > 0.0
    u = rs.random_u(len(xyz)) * 1e-3
    ref, scale = th.mesh_resultants(xyz, tri, quad, u, tt, qt, ALPHA, sec=sec, sec_alpha=sa)
    ratio = th.bound_ratio(fs.element_resultants(u), ref, scale)
    print("heated shell  %-24s random u: max |res - ref| / (1e-12 scale) = %.3e" % (name, ratio))
    assert ratio <= 1.0
    # cleared: the instantiations without temperatures, bitwise what a context without the new calls returns
    fs.set_thermal(None, None)
    plain = _context(xyz, tri, quad, sec)
    np.testing.assert_array_equal(fs.element_resultants(u), plain.element_resultants(u))
    plain.close()
    fs.close()


def test_a_heated_panel_held_statically_determinately_takes_the_free_state():
    """End to end: the isosceles panel held at six dofs (onto the values of u_free there), heated with uniform (Tm, Tg), solved.
    The route of existing code -- the same T fed in as nodal loads through set_loads -- is run beside it: F and the solution of
    the two agree as numbers (the bar of test_static_solve_equals_the_solve_under_the_load_vector), and so does their distance
    from u_free, which is printed."""
    xyz, tri = th.isosceles_panel()
    n, nx = len(xyz), 6
    mask = np.zeros(n, np.uint8)
    mask[0] = 0x07                 # u, v, w at the corner (0, 0)
    mask[nx] = 0x06                # v, w at the corner (lx, 0)
    mask[n - 1 - nx] = 0x04        # w at the corner (0, ly)
    assert xyz[nx, 1] == 0.0 and xyz[n - 1 - nx, 0] == 0.0 and xyz[n - 1 - nx, 1] > 0.0
    u_free = th.free_state(xyz, ALPHA, rs.T, TM, TG)
    temps = np.tile([TM, TG], (len(tri), 1))
    out = []
    for _ in range(2):
        fs = _context(xyz, tri, None)
        fs.set_dirichlet(mask)
        fs.set_preconditioner("jacobi")
        fs.set_prescribed(u_free)
        out.append(fs)
    fa, fb = out
    fa.set_expansion(ALPHA)
    fa.set_thermal(temps)
    Tv = fa.thermal_load_vector()
    fb.set_loads(Tv)
    ua, ia = fa.solve(rtol=1e-13, max_it=200000)
    ub, ib = fb.solve(rtol=1e-13, max_it=200000)
    assert ia["converged"] == 1 and ia["iterations"] == ib["iterations"]
    np.testing.assert_array_equal(fa.export_bsr()[3], fb.export_bsr()[3])
    np.testing.assert_array_equal(ua, ub)
    size = np.abs(u_free).max(axis=0)
    ea, eb = np.abs(ua - u_free).max(axis=0) / size[[0, 1, 2, 3, 4, 4]], np.abs(ub - u_free).max(axis=0) / size[[0, 1, 2, 3, 4, 4]]
    print("end to end: max |u - u_free| / max |u_free| per component, thermal %s, nodal route %s" % (ea, eb))
    assert np.array_equal(ea, eb)
    # the reactions of the two routes are the same numbers; the stress of the solved state, which only the thermal context
    # knows to be free, is printed against its scale (what a CG solution at rtol 1e-13 leaves)
    np.testing.assert_array_equal(fa.reactions(), fb.reactions())
    res = fa.element_resultants()
    _, res_scale = th.mesh_resultants(xyz, tri, None, u_free, temps, None, ALPHA)
    print("end to end: max |N, M, vm| of the solved state / scale = %.3e" % (np.abs(res)[res_scale > 0] / res_scale[res_scale > 0]).max())
    fa.close()
    fb.close()


# ------------------------------------------------------------------ 4. geometric stiffness and buckling

@pytest.mark.parametrize("kind", ["t", "q"])
def test_geometric_product_of_the_clamped_state_is_that_of_the_contraction(kind):
    """K_G with temperatures in force and u = 0 equals, to 1e-12 of the row scales, K_G without temperatures from
    u_c = -alpha Tm (x - x0): the same membrane forces, -N_T, by two routes"""
    xyz, tri, quad = bk.plate(6, kind)
    n = len(xyz)
    nt, nq = _counts(tri, quad)
    Tm = 90.0
    fs = _context(xyz, tri, quad)
    u_c = np.zeros((n, 6))
    u_c[:, 0] = -ALPHA * Tm * (xyz[:, 0] - 0.3)
    u_c[:, 1] = -ALPHA * Tm * (xyz[:, 1] - 0.6)
    X = np.random.default_rng(31).uniform(-1.0, 1.0, (5, n, 6))
    Y_cold = fs.geometric_product(u_c, X)
    fs.set_expansion(ALPHA)
    fs.set_thermal(np.tile([Tm, 7.0], (nt, 1)) if nt else None, np.tile([Tm, 7.0], (nq, 1)) if nq else None)  # (a gradient does not show in N)
    Y_hot = fs.geometric_product(np.zeros((n, 6)), X)
    _, Ta = bk.product(n, bk.element_coefficients(xyz, tri, quad, u_c, rs.NU, rs.E, rs.T), X)
    ratio = bk.bound_ratio(Y_hot, Y_cold, Ta)
    print("geometric product, plate of %s: max |Y_hot - Y_cold| / (1e-12 T_a) = %.3e" % ("triangles" if kind == "t" else "quadrilaterals", ratio))
    assert ratio <= 1.0
    assert np.abs(Y_hot[:, :, :3]).max() > 0.0
    fs.close()


def test_thermal_buckling_of_a_restrained_plate():
    """A simply supported square plate with in-plane restrained edges under uniform Tm: the load factors of femshell_buckling with
    temperatures in force (u = 0: nothing moves) against those of the same mesh without temperatures, u_c = -alpha Tm (x - x0)
    prescribed on the boundary and solved through the existing path -- equal to the buckling tolerance the calls were given, with
    the factor 4 of tests/test_gpu_buckling.py.  The plate formula 2 pi^2 D / (a^2 N_T) is printed beside the lowest factor."""
    tol, n_modes, guard = 1e-8, 3, 3
    nu, E, t = 0.3, 2.1e5, 0.02
    Tm = 100.0
    xyz, tri, _ = bk.plate(8, "t")
    n = len(xyz)
    edge = bk.boundary(xyz)
    mask = np.zeros(n, np.uint8)
    mask[edge] = 0x07
    hot = _context(xyz, tri, None, material=(nu, E, t))
    hot.set_dirichlet(mask)
    hot.set_preconditioner("jacobi")
    hot.set_expansion(ALPHA)
    hot.set_thermal(np.tile([Tm, 0.0], (len(tri), 1)))
    lam_hot, _, info_hot = hot.buckling(n_modes=n_modes, guard=guard, tol=tol, u=np.zeros((n, 6)))
    cold = _context(xyz, tri, None, material=(nu, E, t))
    cold.set_dirichlet(mask)
    cold.set_preconditioner("jacobi")
    u_c = np.zeros((n, 6))
    u_c[:, :2] = -ALPHA * Tm * (xyz[:, :2] - 0.5)
    cold.set_prescribed(u_c)
    _, info = cold.solve(rtol=1e-13, max_it=200000)
    assert info["converged"] == 1
    lam_cold, _, info_cold = cold.buckling(n_modes=n_modes, guard=guard, tol=tol)
    assert info_hot["converged"] == n_modes and info_cold["converged"] == n_modes
    formula = 2.0 * np.pi ** 2 * bk.plate_D(E, nu, t) / (E * t * ALPHA * Tm / (1.0 - nu))
    print("thermal buckling: factors %s (heated) %s (prescribed contraction); plate formula 2 pi^2 D / (a^2 N_T) = %.6f" % (lam_hot, lam_cold, formula))
    for j in range(n_modes):
        assert abs(lam_hot[j] - lam_cold[j]) <= 4.0 * tol * abs(lam_hot[j]), (j, lam_hot, lam_cold)
    assert lam_hot[0] > 0.0  # heating compresses a restrained plate
    hot.close()
    cold.close()


# ------------------------------------------------------------------ 5. refusals

def test_refusals_leave_the_context_usable_and_the_temperatures_in_force():
    xyz, tri = pr.panel(lift=True)
    mask = np.zeros(len(xyz), np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    tt, _ = th.random_temps(len(tri), 0, seed=9)
    dp = ctypes.POINTER(ctypes.c_double)
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    # no mesh
    with pytest.raises(pkg.FemShellError) as info:
        fs.set_thermal(None, None)
    assert info.value.code == -1
    with pytest.raises(pkg.FemShellError) as info:
        fs.set_expansion(ALPHA)
    assert info.value.code == -1
    rc = fs._L.femshell_set_thermal(fs._h, tt.ctypes.data_as(dp), None)
    assert rc == -1 and b"femshell_set_mesh first" in fs._L.femshell_last_error()
    with pytest.raises(pkg.FemShellError):
        fs.thermal_load_vector()
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(mask)
    L = np.random.default_rng(2).uniform(-1.0, 1.0, (len(xyz), 6))
    fs.set_loads(L)
    # temperatures before alpha
    with pytest.raises(pkg.FemShellError) as info:
        fs.set_thermal(tt)
    assert info.value.code == -1 and "femshell_set_expansion" in str(info.value)
    assert not fs.thermal_load_vector().any()
    # a non-finite alpha, a section count that does not match
    for bad in (np.nan, np.inf):
        with pytest.raises(pkg.FemShellError) as info:
            fs.set_expansion(bad)
        assert info.value.code == -1
    with pytest.raises(pkg.FemShellError) as info:
        fs.set_expansion(0.0, [1e-5, 2e-5])
    assert info.value.code == -1
    fs.set_expansion(ALPHA)
    fs.set_thermal(tt)
    Tv = fs.thermal_load_vector()
    fs.assemble()
    F = fs.export_bsr()[3]
    np.testing.assert_array_equal(F, _expected_F(mask, L + Tv))
    for bad_value in (np.nan, np.inf):
        bad = tt.copy()
        bad[len(bad) // 2, 1] = bad_value
        with pytest.raises(pkg.FemShellError) as info:
            fs.set_thermal(bad)
        assert info.value.code == -1
        with pytest.raises(pkg.FemShellError):
            fs.set_expansion(bad_value)
        with pytest.raises(pkg.FemShellError):
            fs.set_expansion(0.0, [1e-5])
        np.testing.assert_array_equal(fs.thermal_load_vector(), Tv)
        np.testing.assert_array_equal(fs.export_bsr()[3], F)
    # set_density does not touch them; set_sections forgets alpha and with it the temperatures: the loads are the nodal ones again
    fs.set_density(7.8e-3)
    np.testing.assert_array_equal(fs.thermal_load_vector(), Tv)
    sections = [[0.3, 2e5, 0.05], [0.25, 7e4, 0.1]]
    fs.set_sections(sections, np.arange(len(tri)) % 2, None)
    assert not fs.thermal_load_vector().any()
    fs.assemble()
    np.testing.assert_array_equal(fs.export_bsr()[3], _expected_F(mask, L))
    with pytest.raises(pkg.FemShellError):
        fs.set_thermal(tt)  # alpha went with the sections
    with pytest.raises(pkg.FemShellError):
        fs.set_expansion(0.0, SEC_ALPHA)  # three values for two sections
    fs.set_expansion(0.0, [1e-5, 2e-5])
    fs.set_thermal(tt)
    sec = (sections, np.arange(len(tri)) % 2, None)
    T_ref, scale = th.load_vector(xyz, tri, None, tt, None, 0.0, sec=sec, sec_alpha=[1e-5, 2e-5])
    assert th.bound_ratio(fs.thermal_load_vector(), T_ref, scale) <= 1.0
    fs.set_sections(None)  # clearing the sections forgets them as well
    assert not fs.thermal_load_vector().any()
    # set_mesh forgets temperatures and alpha (and the nodal loads)
    fs.set_expansion(ALPHA)
    fs.set_thermal(tt)
    np.testing.assert_array_equal(fs.thermal_load_vector(), Tv)
    fs.set_mesh(xyz, tri)
    assert not fs.thermal_load_vector().any()
    with pytest.raises(pkg.FemShellError):
        fs.set_thermal(tt)
    fs.set_dirichlet(mask)
    fs.set_loads(L)
    fs.assemble()
    np.testing.assert_array_equal(fs.export_bsr()[3], _expected_F(mask, L))
    fs.close()


# ------------------------------------------------------------------ 6. the timing hook

@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24", "panel_three_sections"])
def test_time_kernel_reports_the_bytes_of_the_model(name):
    """per listed element 16 + 4 + 16 bytes (4 more with sections), 24 per node, 96 per owned row; the loads in force are not
    disturbed"""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    assert not env
    nt, nq = _counts(tri, quad)
    fs = _context(xyz, tri, quad, sec)
    ms, by = fs.time_kernel(pkg.KERNEL_ELEMENT_THERMAL, reps=3)  # a mesh is all it needs
    assert ms > 0.0
    n = len(xyz)
    assert by == th.model_bytes(el.listed_elements(n, tri, quad), n, n, sections=sec is not None)
    mask = _mask(n)
    fs.set_dirichlet(mask)
    L = np.random.default_rng(2).uniform(-1.0, 1.0, (n, 6))
    fs.set_loads(L)
    _expand(fs, sec)
    fs.set_thermal(*th.random_temps(nt, nq))
    Tv = fs.thermal_load_vector()
    fs.assemble()
    F = fs.export_bsr()[3]
    ms, by2 = fs.time_kernel(pkg.KERNEL_ELEMENT_THERMAL, reps=3)
    assert ms > 0.0 and by2 == by
    np.testing.assert_array_equal(fs.thermal_load_vector(), Tv)
    np.testing.assert_array_equal(fs.export_bsr()[3], F)
    np.testing.assert_array_equal(F, _expected_F(mask, L + Tv))
    fs.close()


# ------------------------------------------------------------------ 7. slice walk and ranks (child processes)

WORKER = os.path.join(ROOT, "tests", "helpers", "thermal_worker.py")
FAKE_DIR = os.path.join(ROOT, "tests", "helpers", "fake_rccl")
CHILD_TIMEOUT = 240


def run_ranks(world, tmp_path, tag, extra_env=None):
    """the launch pattern of tests/test_gpu_element_loads.py on the thermal worker"""
    subprocess.check_call(["make", "-C", FAKE_DIR, "-s"])
    env = dict(os.environ, FEMSHELL_RCCL_LIB=os.path.join(FAKE_DIR, "libfake_rccl.so"))
    env.pop("FEMSHELL_SLICE_GRID", None)
    env.update(extra_env or {})
    uid = str(tmp_path / ("uid_%s.npy" % tag))
    outs = [str(tmp_path / ("out_%s_%d.npz" % (tag, r))) for r in range(world)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), uid, outs[r]], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(out.decode(errors="replace"))
    for r, p in enumerate(procs):
        assert p.returncode == 0, "rank %d failed:\n%s" % (r, "\n".join("--- rank %d\n%s" % (q, logs[q][-1500:]) for q in range(world)))
    return [dict(np.load(o)) for o in outs]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One child per grid setting, then the two ranks, one after another; the first child that does not exit 0 ends the module
    (nothing more is started on the GPU behind a child that failed)."""
    tmp = tmp_path_factory.mktemp("thermal")
    got = {}
    for grid in ("default", "8"):
        got[grid] = run_ranks(1, tmp, "grid" + grid, {} if grid == "default" else {"FEMSHELL_SLICE_GRID": grid})[0]
    got["ranks"] = run_ranks(2, tmp, "ranks")
    return got


def _reference_of_the_worker():
    from tests.helpers.thermal_worker import ALPHA as alpha, problem
    xyz, tri, tt, tl, mask, nodal = problem()
    T_ref, scale = th.load_vector(xyz, tri, None, tt, None, alpha)
    return mask, nodal, T_ref, scale


def test_more_slices_than_workgroups_give_the_bits_of_the_default_grid(runs):
    mask, nodal, T_ref, scale = _reference_of_the_worker()
    base = runs["default"]
    assert int(base["slices"]) == 40 and len(base["T"]) == 1271 and int(base["same"]) == 1
    assert th.bound_ratio(base["T"], T_ref, scale) <= 1.0
    np.testing.assert_array_equal(base["F"], _expected_F(mask, (nodal + base["S"]) + base["T"]))
    run = runs["8"]
    assert (int(run["slices"]) + 7) // 8 > 1  # a workgroup took a second slice
    assert int(run["same"]) == 1
    np.testing.assert_array_equal(run["T"], base["T"])
    np.testing.assert_array_equal(run["F"], base["F"])


def test_two_ranks_on_one_gpu_gather_the_load_vector_of_the_single_rank_run(runs):
    """both ranks return the same gathered T; it agrees with the single-rank T to 1e-13 of the scale (a rank sums a row over its own
    list, whose order may differ from the single rank's); every rank's rows of F are fl(fl(nodal + S) + T) of its own vectors"""
    mask, nodal, T_ref, scale = _reference_of_the_worker()
    single, ranks = runs["default"], runs["ranks"]
    ranks = sorted(ranks, key=lambda q: int(q["begin"]))
    assert int(ranks[0]["begin"]) == 0 and int(ranks[0]["end"]) == int(ranks[1]["begin"]) and int(ranks[1]["end"]) == len(single["T"])
    assert 0 < int(ranks[0]["end"]) < len(single["T"])
    np.testing.assert_array_equal(ranks[0]["T"], ranks[1]["T"])
    ratio = th.bound_ratio(ranks[0]["T"], single["T"], scale, tol=1e-13)
    print("two ranks: max |T - T_single| / (1e-13 scale) = %.3e" % ratio)
    assert ratio <= 1.0
    assert th.bound_ratio(ranks[0]["T"], T_ref, scale) <= 1.0
    want = _expected_F(mask, (nodal + ranks[0]["S"]) + ranks[0]["T"])
    for r in ranks:
        assert int(r["same"]) == 1
        np.testing.assert_array_equal(r["F"], want[6 * int(r["begin"]):6 * int(r["end"])])
