"""Elastic supports on the device (femshell_set_foundation, femshell_set_springs, femshell_support_stiffness,
femshell_support_forces) against tests/helpers/elastic_support.py, the longdouble reference tests/test_elastic_support_cpu.py pins,
and what the library promises of them: K in HBM is K + mask(K_sup) after every assembly, one addition per entry of the diagonal
blocks, and every consumer of K, of the right-hand side and of the reactions sees the supported shell."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import dynamics, elastic_support as es, element_loads as el, modal, oracle, prescribed as pr, resultants as rs
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

TINY = 1e-12
RHO = 7.8e-3
INVALID = -1


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


def _counts(tri, quad):
    return (0 if tri is None else len(tri)), (0 if quad is None else len(quad))


def _context(xyz, tri, quad, sec=None, pc="jacobi"):
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    fs.set_mesh(xyz, tri, quad)
    if sec is not None:
        fs.set_sections(sec[0], sec[1], sec[2])
    fs.set_preconditioner(pc)
    return fs


def _mask(n):
    mask = np.zeros(n, np.uint8)
    mask[::3] = 0x15
    mask[0] = 0x3F
    return mask


def _clamped(xyz):
    mask = np.zeros(len(xyz), np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    return mask


def _supports(xyz, tri, quad=None, seed=5):
    nt, nq = _counts(tri, quad)
    tk, qk = es.random_moduli(nt, nq, seed=seed)
    return tk, qk, es.random_springs(len(xyz), seed=seed + 1)


def _material():
    return oracle.material(rs.NU, rs.E, rs.T)


# ------------------------------------------------------------------ 1. the table against the reference

@pytest.mark.parametrize("name", list(rs.device_meshes()))
def test_support_table_matches_the_reference(name, monkeypatch):
    """Seeded random (kn, kt) and springs on a third of the nodes: per node and word |S - S_ref| <= 1e-12 T_a, T_a = sum over the
    row's elements of (kn + kt) |d1| |d2| + the node's largest spring.  Each word of B_e costs a handful of roundings and the
    list-order sum of at most 765 terms about (n_e + 12) eps: the argument and the bar of the element loads.  Two calls give the
    same bits; one kind alone, clearing and a Dirichlet set do not show in the table."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nt, nq = _counts(tri, quad)
    n = len(xyz)
    fs = _context(xyz, tri, quad, sec)
    assert fs.support_stiffness().shape == (n, 9) and not fs.support_stiffness().any()  # none set yet
    tk, qk, springs = _supports(xyz, tri, quad)
    fs.set_foundation(tk, qk)
    fs.set_springs(*es.nodes_of(springs))
    S = fs.support_stiffness()
    S_ref, T = es.table(xyz, tri, quad, tk, qk, springs)
    ratio = es.bound_ratio(S, S_ref, T)
    print("elastic_support_vs_reference %-28s elements %5d  max |S - S_ref| / (1e-12 T_a) = %.3e" % (name, nt + nq, ratio))
    assert ratio <= 1.0
    assert np.abs(S[:, :6]).max() > 0.0 and np.array_equal(S[:, 6:], springs[:, 3:])
    assert np.array_equal(S, fs.support_stiffness())
    fs.set_dirichlet(_mask(n))
    assert np.array_equal(S, fs.support_stiffness())
    fs.set_springs(springs)  # the dense form
    assert np.array_equal(S, fs.support_stiffness())
    # one set alone, one kind alone
    fs.set_springs(None)
    F_only = fs.support_stiffness()
    assert es.bound_ratio(F_only, es.table(xyz, tri, quad, tk, qk)[0], T) <= 1.0 and not F_only[:, 6:].any()
    if nt and nq:
        fs.set_foundation(tk, None)
        assert es.bound_ratio(fs.support_stiffness(), es.table(xyz, tri, quad, tk, None)[0], T) <= 1.0
        fs.set_foundation(None, qk)
        assert es.bound_ratio(fs.support_stiffness(), es.table(xyz, tri, quad, None, qk)[0], T) <= 1.0
    fs.set_foundation(None, None)
    assert not fs.support_stiffness().any()
    fs.set_springs(springs)
    only = fs.support_stiffness()
    assert np.array_equal(only[:, :3], springs[:, :3]) and np.array_equal(only[:, 6:], springs[:, 3:]) and not only[:, 3:6].any()
    fs.set_foundation(tk, qk)
    assert np.array_equal(S, fs.support_stiffness())
    fs.close()


def test_wrong_lengths_are_refused_by_the_binding():
    xyz, tri, quad = rs.device_meshes()["mixed_petals24"]()[:3]
    fs = _context(xyz, tri, quad)
    with pytest.raises(ValueError):
        fs.set_foundation(np.zeros((len(tri) + 1, 2)), None)
    with pytest.raises(ValueError):
        fs.set_foundation(None, np.zeros((len(quad) - 1, 2)))
    with pytest.raises(ValueError):
        fs.set_springs(np.zeros((len(xyz) - 1, 6)))
    with pytest.raises(ValueError):
        fs.set_springs([0, 1], np.zeros((3, 6)))
    fs.close()


# ------------------------------------------------------------------ 2. K in HBM

@pytest.mark.parametrize("name", ["lifted_panel", "lifted_panel_full_storage"])
def test_the_matrix_in_hbm_is_k_plus_the_masked_supports(name, monkeypatch):
    """export_bsr with and without supports under a Dirichlet set with partly fixed nodes: the off-diagonal blocks and F are
    bitwise equal, every entry of a diagonal block is fl(K_ij + S_ij) at free-free pairs and unchanged where a dof is fixed, the
    exported block is symmetric bit for bit; spmv(x) - spmv_without(x) = mask(K_sup x) to 1e-12 of the row scale."""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = len(xyz)
    mask = _mask(n)
    loads = np.random.default_rng(4).uniform(-1.0, 1.0, (n, 6))
    tk, qk, springs = _supports(xyz, tri, quad)
    out = []
    for supported in (False, True):
        fs = _context(xyz, tri, quad, sec)
        fs.set_dirichlet(mask)
        fs.set_loads(loads)
        if supported:
            fs.set_foundation(tk, qk)
            fs.set_springs(springs)
        fs.assemble()
        x = rs.random_u(n).ravel()
        out.append((fs.export_bsr(), fs.spmv(x), fs.support_stiffness()))
        fs.close()
    (r0, c0, v0, F0), y0, _ = out[0]
    (r1, c1, v1, F1), y1, S = out[1]
    assert np.array_equal(r0, r1) and np.array_equal(c0, c1) and np.array_equal(F0, F1)
    d = es.diagonal_slots(r0, c0)
    off = np.ones(len(c0), bool)
    off[d] = False
    np.testing.assert_array_equal(v0[off], v1[off])
    add = es.masked_blocks(S, mask)
    assert (add != 0).sum() > n
    np.testing.assert_array_equal(v1[d], v0[d] + add)
    fixed = pr.fixed_dofs(mask).reshape(n, 6)
    touched = ~(fixed[:, :, None] | fixed[:, None, :])
    np.testing.assert_array_equal(v1[d][~touched], v0[d][~touched])
    np.testing.assert_array_equal(v1[d], np.transpose(v1[d], (0, 2, 1)))
    scale = pr.row_scale((r1, c1, v1), x)
    ratio = (np.abs((y1 - y0).reshape(n, 6) - es.apply(S, x, mask)).max(axis=1) / (TINY * scale)).max()
    print("spmv with supports %-28s: |dy - mask(K_sup x)| / (1e-12 row scale) = %.2e" % (name, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------ 3. rigid translation

@pytest.mark.parametrize("pc", ["jacobi", "amg"])
@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24"])
def test_a_free_shell_on_an_isotropic_foundation_translates_rigidly(name, pc):
    """no Dirichlet dof, k = 1e4 on every element, loads k A_a d: u = d without rotation to 1e-10 max |d| (the bar of
    test_rigid_translation_moves_every_node_and_loads_no_support; the reference alone reaches 4e-12,
    tests/test_elastic_support_cpu.py), and support_forces balances the loads column by column to 1e-9 sum k A |d|"""
    xyz, tri, quad = rs.device_meshes()[name]()[:3]
    nt, nq = _counts(tri, quad)
    n = len(xyz)
    k, d = 1e4, np.array([1.0, 2.0, 3.0]) * 1e-3
    tk, qk = (np.full((nt, 2), k) if nt else None), (np.full((nq, 2), k) if nq else None)
    S_ref, _ = es.table(xyz, tri, quad, tk, qk)
    loads = np.zeros((n, 6))
    loads[:, :3] = S_ref[:, :1] * d
    fs = _context(xyz, tri, quad, pc=pc)
    fs.set_loads(loads)
    fs.set_foundation(tk, qk)
    u, info = fs.solve(rtol=1e-13, max_it=50000)
    err = max(np.abs(u[:, :3] - d).max(), np.abs(u[:, 3:]).max()) / np.abs(d).max()
    f = fs.support_forces()
    balance = np.abs((f + loads)[:, :3].sum(axis=0)).max()
    total = (S_ref[:, 0] * np.abs(d).sum()).sum()
    print("rigid translation on a foundation %-16s %-6s iterations %5d: max |u - d| / max |d| = %.2e, balance / (1e-9 sum k A |d|) = %.2e"
          % (name, pc, info["iterations"], err, balance / (1e-9 * total)))
    assert info["converged"] == 1
    assert err <= 1e-10
    assert balance <= 1e-9 * total and not f[:, 3:].any()
    assert np.array_equal(f, fs.support_forces(u))
    fs.close()


# ------------------------------------------------------------------ 4. the solve against the reference

@pytest.mark.parametrize("pc", ["jacobi", "amg"])
def test_supported_solve_matches_the_reference(pc):
    """the clamped lifted panel under nodal loads with a random foundation and springs against the refined direct solve of
    K_c + mask(K_sup) from the oracle: 1e-10, the bar of test_prescribed_solve_matches_the_reference"""
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = _clamped(xyz)
    loads = np.random.default_rng(8).uniform(-1.0, 1.0, (n, 6)) * [5.0, 5.0, 0.5, 0.1, 0.1, 0.1]
    tk, _, springs = _supports(xyz, tri)
    fs = _context(xyz, tri, None, pc=pc)
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    _, bare = fs.solve(rtol=1e-13, max_it=50000)
    fs.set_foundation(tk)
    fs.set_springs(springs)
    u, info = fs.solve(rtol=1e-13, max_it=50000)
    S_ref, _ = es.table(xyz, tri, None, tk, None, springs)
    _, K_c = pr.matrices(xyz, tri, None, _material(), mask)
    rhs = np.where(pr.fixed_dofs(mask), 0.0, loads.ravel())
    u_ref = oracle.refined_solve(*es.add_to_bsr(K_c, S_ref, mask), rhs)
    err = rel(u, u_ref)
    print("supported solve %-6s: iterations %d with supports, %d without, error vs reference %.2e" % (pc, info["iterations"], bare["iterations"], err))
    assert info["converged"] == 1
    assert err <= 1e-10
    fs.close()


# ------------------------------------------------------------------ 5. prescribed values and reactions

def test_prescribed_values_and_reactions_see_the_supports():
    """F = mask(loads - (K_unc + K_sup) u_bar) to 1e-12 scale(u_bar); r against pr.reactions with K_unc + K_sup to 1e-12 S_a; the
    force columns of r + support_forces + loads sum to zero to 1e-12 sum S_a; the NULL forms give the bits of the explicit ones"""
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = _clamped(xyz)
    tip = pr.edge_nodes(xyz, 0, pr.LX)
    mask[tip] = 0x04
    ubar = np.zeros((n, 6))
    ubar[tip, 2] = 0.01
    loads = np.random.default_rng(9).uniform(-1.0, 1.0, (n, 6)) * [5.0, 5.0, 0.5, 0.1, 0.1, 0.1]
    tk, _, springs = _supports(xyz, tri)
    springs[tip[0]] = [2e3, 1e3, 3e3, 40.0, 50.0, 60.0]  # a spring under a prescribed dof
    fs = _context(xyz, tri, None)
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.set_prescribed(ubar)
    fs.set_foundation(tk)
    fs.set_springs(springs)
    u, info = fs.solve(rtol=1e-13, max_it=50000)
    assert info["converged"] == 1 and np.array_equal(u[tip, 2], np.full(len(tip), 0.01))
    S = fs.support_stiffness()
    K_unc, _ = pr.matrices(xyz, tri, None, _material(), mask)
    K_sum = es.add_to_bsr(K_unc, S)
    fixed = pr.fixed_dofs(mask)
    F = fs.export_bsr()[3]
    F_ref = np.where(fixed, 0.0, loads.ravel() - oracle.spmv(*K_sum, ubar.ravel()))
    scale = pr.row_scale(K_sum, ubar)  # (zero on the rows u_bar does not reach: F is the masked loads there, bit for bit)
    diff = np.abs(F - F_ref).reshape(n, 6).max(axis=1)
    assert (scale > 0).any() and not diff[scale == 0].any()
    ratio_F = (diff[scale > 0] / (TINY * scale[scale > 0])).max()
    assert not np.array_equal(F, np.where(fixed, 0.0, loads.ravel()))  # u_bar shows
    r = fs.reactions()
    Sa = pr.row_scale(K_sum, u)
    ratio_r = (np.abs(r - pr.reactions(K_sum, u, loads)).max(axis=1) / (TINY * Sa)).max()
    f = fs.support_forces()
    assert np.abs(f + es.apply(S, u)).max() <= TINY * Sa.max()
    balance = np.abs((r + f + loads)[:, :3].sum(axis=0)).max()
    print("supports with prescribed values: |F - F_ref| / (1e-12 scale) = %.2e, |r - r_ref| / (1e-12 S_a) = %.2e, balance / (1e-12 sum S_a) = %.2e"
          % (ratio_F, ratio_r, balance / (TINY * Sa.sum())))
    assert ratio_F <= 1.0 and ratio_r <= 1.0
    assert balance <= TINY * Sa.sum()
    assert np.abs(r.ravel()[~fixed]).max() <= 1e-9 * Sa.max()  # the negative residual at the free dofs
    assert np.array_equal(fs.reactions(u), r) and np.array_equal(fs.support_forces(u), f)
    fs.close()


# ------------------------------------------------------------------ 6. state

def test_a_change_of_the_supports_makes_the_next_solve_assemble_again():
    """setting, replacing or clearing either set: assemble_seconds > 0 and pc_setup_seconds > 0 at the next solve, 0 at the one
    after; after clearing, K and the solution are those of a fresh context bit for bit; set_mesh forgets both sets, set_sections
    and set_dirichlet keep them; after a shifted modes call the supports are back in K"""
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = _clamped(xyz)
    loads = np.random.default_rng(8).uniform(-1.0, 1.0, (n, 6))
    tk, _, springs = _supports(xyz, tri)

    def fresh():
        fs = _context(xyz, tri, None, pc="amg")
        fs.set_dirichlet(mask)
        fs.set_loads(loads)
        return fs

    def solve_twice(fs, what):
        u, a = fs.solve(rtol=1e-12, max_it=5000)
        _, b = fs.solve(rtol=1e-12, max_it=5000)
        assert a["converged"] == 1 and a["assemble_seconds"] > 0.0 and a["pc_setup_seconds"] > 0.0, (what, a)
        assert b["assemble_seconds"] == 0.0 and b["pc_setup_seconds"] == 0.0, (what, b)
        return u

    base = fresh()
    u0 = solve_twice(base, "fresh")
    K0 = base.export_bsr()
    fs = fresh()
    solve_twice(fs, "fresh")
    fs.set_foundation(tk)
    u1 = solve_twice(fs, "foundation set")
    fs.set_foundation(2.0 * tk)
    u2 = solve_twice(fs, "foundation replaced")
    fs.set_springs(springs)
    u3 = solve_twice(fs, "springs set")
    fs.set_springs(2.0 * springs)
    solve_twice(fs, "springs replaced")
    assert not np.array_equal(u0, u1) and not np.array_equal(u1, u2) and not np.array_equal(u2, u3)
    fs.set_foundation(None, None)
    solve_twice(fs, "foundation cleared")
    fs.set_springs(None)
    u4 = solve_twice(fs, "springs cleared")
    for a, b in zip(fs.export_bsr(), K0):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(u4, u0)
    # set_sections and set_dirichlet keep the sets; a shifted modes call leaves them in K
    fs.set_foundation(tk)
    fs.set_springs(springs)
    S = fs.support_stiffness()
    fs.set_dirichlet(_mask(n))
    fs.set_sections([[0.3, 2e5, 0.05], [0.25, 7e4, 0.1]], np.arange(len(tri)) % 2, None)
    np.testing.assert_array_equal(fs.support_stiffness(), S)
    fs.set_sections(None)
    fs.set_dirichlet(mask)
    fs.assemble()
    K1 = fs.export_bsr()
    d = es.diagonal_slots(K0[0], K0[1])
    np.testing.assert_array_equal(K1[2][d], K0[2][d] + es.masked_blocks(S, mask))
    fs.set_density(RHO)
    fs.modes(2, tol=1e-4, shift=10.0, max_it=300)
    fs.assemble()  # (leaving a shifted run makes K stale: the assembly that follows adds the supports again)
    for a, b in zip(fs.export_bsr(), K1):
        np.testing.assert_array_equal(a, b)
    # set_mesh forgets both
    fs.set_mesh(xyz, tri)
    assert not fs.support_stiffness().any()
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.assemble()
    for a, b in zip(fs.export_bsr(), K0):
        np.testing.assert_array_equal(a, b)
    fs.close()
    base.close()


# ------------------------------------------------------------------ 7. downstream: modes and dynamics

def test_modes_of_the_supported_panel():
    """a free-floating panel made definite by its supports alone, no shift: the four lowest eigenvalues against the dense
    reference of tests/helpers/modal.py on the exported K + mask(K_sup) and the lumped mass, to 1e-8 lam as tests/test_gpu_modal.py"""
    xyz, tri = pr.panel(lift=True)
    tk, _, springs = _supports(xyz, tri)
    fs = _context(xyz, tri, None)
    fs.set_density(RHO)
    fs.set_foundation(tk)
    fs.set_springs(springs)
    fs.assemble()
    r, c, v, _ = fs.export_bsr()
    mass = dynamics.lumped_mass(xyz, tri, None, RHO, rs.T)
    dmask = np.zeros(len(xyz), np.uint8)
    lam_ref, _ = modal.reference(dynamics.to_matrix((r, c, v)), mass, dmask, 8, 0.0)
    lam, _, res, info = fs.modes(4, tol=1e-6, max_it=500)
    print("modes of the supported panel: lam %s, worst deviation %.2e" % (lam, (np.abs(lam - lam_ref[:4]) / lam_ref[:4]).max()))
    assert info["converged"] == 4 and lam_ref[0] > 0.0
    assert (np.abs(lam - lam_ref[:4]) <= 1e-8 * lam_ref[:4]).all()
    fs.close()


def test_one_newmark_step_with_supports():
    """one step from rest against tests/helpers/dynamics.py fed the exported K + mask(K_sup): 1e-9 of max |u|, the bar per step of
    tests/test_gpu_dynamics.py; the setters are refused while dynamics is active"""
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = _clamped(xyz)
    loads = np.random.default_rng(8).uniform(-1.0, 1.0, (n, 6)) * [5.0, 5.0, 0.5, 0.1, 0.1, 0.1]
    tk, _, springs = _supports(xyz, tri)
    fs = _context(xyz, tri, None)
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.set_density(RHO)
    fs.set_foundation(tk)
    fs.set_springs(springs)
    fs.assemble()
    K = dynamics.to_matrix(fs.export_bsr())
    mass = dynamics.lumped_mass(xyz, tri, None, RHO, rs.T)
    dt = 1e-3
    ref = dynamics.Newmark(K, mass, mask, dt)
    free = dynamics.free_dofs(mask, n)
    ref.begin(loads.ravel() * free)
    fs.dynamics_begin(dt)
    S = fs.support_stiffness()
    for call in (lambda: fs.set_foundation(tk), lambda: fs.set_springs(springs), lambda: fs.set_foundation(None, None), lambda: fs.set_springs(None)):
        with pytest.raises(pkg.FemShellError) as info:
            call()
        assert info.value.code == INVALID
    np.testing.assert_array_equal(fs.support_stiffness(), S)
    assert fs.dynamics_step(rtol=1e-12, max_it=50000)["converged"] == 1
    u = fs.dynamics_state(candidate=True)[0].ravel()
    u_ref = ref.step(loads.ravel())[0]
    worst = np.abs(u - u_ref).max() / np.abs(u_ref).max()
    print("one Newmark step with supports: max |u - u_ref| / max |u| = %.2e" % worst)
    assert np.abs(u_ref).max() > 0.0 and worst <= 1e-9
    fs.dynamics_end()
    fs.close()


# ------------------------------------------------------------------ 8. refusals

def test_refusals_leave_the_context_usable_and_the_supports_in_force():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = _clamped(xyz)
    tk, _, springs = _supports(xyz, tri)
    dp = ctypes.POINTER(ctypes.c_double)
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    # no mesh
    for call in (lambda: fs.set_foundation(None, None), lambda: fs.set_springs(None), fs.support_stiffness, lambda: fs.support_forces(np.zeros((0, 6)))):
        with pytest.raises(pkg.FemShellError) as info:
            call()
        assert info.value.code == INVALID
    rc = fs._L.femshell_set_foundation(fs._h, tk.ctypes.data_as(dp), None)
    assert rc == INVALID and b"femshell_set_mesh first" in fs._L.femshell_last_error()
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(mask)
    fs.set_loads(np.random.default_rng(2).uniform(-1.0, 1.0, (n, 6)))
    with pytest.raises(pkg.FemShellError):  # no solve has run
        fs.support_forces()
    fs.set_foundation(tk)
    fs.set_springs(springs)
    S = fs.support_stiffness()
    u, info = fs.solve(rtol=1e-12, max_it=50000)
    K = fs.export_bsr()
    ids, rows = es.nodes_of(springs)
    bad_calls = []
    for bad_value in (np.nan, np.inf, -1.0):
        bad = tk.copy()
        bad[len(bad) // 2, 1] = bad_value
        bad_calls.append(lambda bad=bad: fs.set_foundation(bad))
        bad = rows.copy()
        bad[len(bad) // 2, 4] = bad_value
        bad_calls.append(lambda bad=bad: fs.set_springs(ids, bad))
    bad_calls.append(lambda: fs.set_springs(np.array([0, n], np.int32), rows[:2]))   # out of range
    bad_calls.append(lambda: fs.set_springs(np.array([0, -1], np.int32), rows[:2]))
    bad_calls.append(lambda: fs.set_springs(np.array([3, 5, 3], np.int32), rows[:3]))  # listed twice
    for call in bad_calls:
        with pytest.raises(pkg.FemShellError) as err:
            call()
        assert err.value.code == INVALID
        np.testing.assert_array_equal(fs.support_stiffness(), S)
    u2, info2 = fs.solve(rtol=1e-12, max_it=50000)
    assert info2["assemble_seconds"] == 0.0  # nothing was made stale
    np.testing.assert_array_equal(u2, u)
    for a, b in zip(fs.export_bsr(), K):
        np.testing.assert_array_equal(a, b)
    fs.close()


# ------------------------------------------------------------------ 9. the timing hook

@pytest.mark.parametrize("name", ["lifted_panel", "mixed_petals24", "coil300"])
def test_time_kernel_reports_the_bytes_of_the_model(name):
    """per listed element 16 + 4 + 16 bytes, 24 per node, 72 per row of the slices; the table in force is not disturbed"""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    assert not env
    n = len(xyz)
    fs = _context(xyz, tri, quad)
    ms, by = fs.time_kernel(pkg.KERNEL_ELASTIC_SUPPORT, reps=3)  # a mesh is all it needs
    assert ms > 0.0
    assert by == es.model_bytes(el.listed_elements(n, tri, quad), n, (n + 31) // 32)
    assert not fs.support_stiffness().any()
    tk, qk, springs = _supports(xyz, tri, quad)
    fs.set_foundation(tk, qk)
    fs.set_springs(springs)
    S = fs.support_stiffness()
    fs.assemble()
    K = fs.export_bsr()
    ms, by2 = fs.time_kernel(pkg.KERNEL_ELASTIC_SUPPORT, reps=3)
    assert ms > 0.0 and by2 == by
    np.testing.assert_array_equal(fs.support_stiffness(), S)
    for a, b in zip(fs.export_bsr(), K):
        np.testing.assert_array_equal(a, b)
    # the timed assembly ends in K + mask(K_sup) as every assembly does
    fs.time_kernel(pkg.KERNEL_ASSEMBLE, reps=2)
    for a, b in zip(fs.export_bsr()[:3], K[:3]):
        np.testing.assert_array_equal(a, b)
    fs.close()


# ------------------------------------------------------------------ 10. slice walk and ranks (child processes)

WORKER = os.path.join(ROOT, "tests", "helpers", "elastic_support_worker.py")
FAKE_DIR = os.path.join(ROOT, "tests", "helpers", "fake_rccl")
CHILD_TIMEOUT = 240


def run_ranks(world, tmp_path, tag, extra_env=None):
    """the launch pattern of tests/test_gpu_element_loads.py on the elastic-support worker"""
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
    tmp = tmp_path_factory.mktemp("elastic_support")
    got = {}
    for grid in ("default", "8", "24"):
        got[grid] = run_ranks(1, tmp, "grid" + grid, {} if grid == "default" else {"FEMSHELL_SLICE_GRID": grid})[0]
    got["ranks"] = run_ranks(2, tmp, "ranks")
    return got


def _reference_of_the_worker():
    from tests.helpers.elastic_support_worker import problem
    xyz, tri, tk, springs, mask, nodal = problem()
    S_ref, T = es.table(xyz, tri, None, tk, None, springs)
    return mask, S_ref, T


def test_more_slices_than_workgroups_give_the_bits_of_the_default_grid(runs):
    mask, S_ref, T = _reference_of_the_worker()
    base = runs["default"]
    assert int(base["slices"]) == 40 and len(base["S"]) == 1271 and int(base["same"]) == 1 and int(base["converged"]) == 1
    assert es.bound_ratio(base["S"], S_ref, T) <= 1.0
    for grid in ("8", "24"):
        run = runs[grid]
        assert (int(run["slices"]) + 7) // 8 > int(grid) // 8  # a workgroup took a second slice
        assert int(run["same"]) == 1
        np.testing.assert_array_equal(run["S"], base["S"], err_msg="grid " + grid)
        np.testing.assert_array_equal(run["diag"], base["diag"], err_msg="grid " + grid)


def test_two_ranks_on_one_gpu_gather_the_table_and_solve_like_the_single_rank(runs):
    """both ranks return the same gathered table; it agrees with the single rank's to 1e-13 T_a (a rank sums a row over its own
    list, whose order may differ from the single rank's); the solutions agree within 1e-10"""
    mask, S_ref, T = _reference_of_the_worker()
    single, ranks = runs["default"], runs["ranks"]
    ranks = sorted(ranks, key=lambda q: int(q["begin"]))
    assert int(ranks[0]["begin"]) == 0 and int(ranks[0]["end"]) == int(ranks[1]["begin"]) and int(ranks[1]["end"]) == len(single["S"])
    assert 0 < int(ranks[0]["end"]) < len(single["S"])
    np.testing.assert_array_equal(ranks[0]["S"], ranks[1]["S"])
    ratio = es.bound_ratio(ranks[0]["S"], single["S"], T, tol=1e-13)
    print("two ranks: max |S - S_single| / (1e-13 T_a) = %.3e" % ratio)
    assert ratio <= 1.0
    assert es.bound_ratio(ranks[0]["S"], S_ref, T) <= 1.0
    for r in ranks:
        assert int(r["same"]) == 1 and int(r["converged"]) == 1
        err = rel(r["u"], single["u"])
        print("two ranks: rank at row %d, solution against the single rank %.2e" % (int(r["begin"]), err))
        assert err <= 1e-10
