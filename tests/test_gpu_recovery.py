"""Nodal stress recovery and the Zienkiewicz-Zhu indicator on the device (femshell_nodal_resultants, FemShell.nodal_resultants)
against tests/helpers/recovery.py, the reference tests/test_recovery_cpu.py pins, within the bounds that module derives."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import element_loads as el, prescribed as pr, recovery as rc, resultants as rs, thermal as th
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()


def _context(xyz, tri, quad, sec=None):
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    fs.set_mesh(xyz, tri, quad)
    if sec is not None:
        fs.set_sections(sec[0], sec[1], sec[2])
    return fs


def _held(name, ref, nodes, elems):
    ratios = ref.ratios(nodes, elems)
    print("nodal_recovery_vs_reference %-28s nodes %5d elements %5d  largest ratio to the bound: tensors %.3e  W %.3e  fold %.3e  e2 %.3e  eta2 %.3e"
          % ((name, len(nodes), len(elems)) + ratios))
    assert max(ratios) <= 1.0, ratios


# ------------------------------------------------------------------ 1. device against reference

@pytest.mark.parametrize("name", list(rc.device_meshes()))
def test_recovery_matches_the_reference(name, monkeypatch):
    """every node word and both element words within the bounds of tests/helpers/recovery.py (tests/test_recovery_cpu.py holds the
    reference's own two evaluations to them on every mesh here); u random in (-1, 1); two calls give the same bits; either output
    alone gives the bits of both together"""
    xyz, tri, quad, sec, env = rc.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fs = _context(xyz, tri, quad, sec)
    u = rs.random_u(len(xyz))
    nodes, elems = fs.nodal_resultants(u)
    assert nodes.shape == (len(xyz), 14) and elems.shape == ((0 if tri is None else len(tri)) + (0 if quad is None else len(quad)), 2)
    again = fs.nodal_resultants(u)
    assert np.array_equal(nodes, again[0]) and np.array_equal(elems, again[1])
    only_n, only_e = np.zeros_like(nodes), np.zeros_like(elems)
    uc = np.ascontiguousarray(u)
    dp = lambda a: a.ctypes.data_as(fs._L.femshell_nodal_resultants.argtypes[1])  # noqa: E731
    assert fs._L.femshell_nodal_resultants(fs._h, dp(uc), dp(only_n), None) == 0
    assert fs._L.femshell_nodal_resultants(fs._h, dp(uc), None, dp(only_e)) == 0
    assert np.array_equal(only_n, nodes) and np.array_equal(only_e, elems)
    ref = rc.Recovery(xyz, tri, quad, u, sec=sec)
    _held(name, ref, nodes, elems)
    assert abs(pkg.relative_error(elems) - rc.relative_error(ref.elems)) <= 1e-9
    fs.close()


def test_fold_measure_of_the_folded_plate():
    """the ridge of two equal panels at a right angle: 1 - cos 45 deg, zero elsewhere, within 32 EPS"""
    xyz, quad, ridge = rc.folded_plate()
    fs = _context(xyz, None, quad)
    nodes, _ = fs.nodal_resultants(rs.random_u(len(xyz)))
    off = np.setdiff1d(np.arange(len(xyz)), ridge)
    assert np.abs(nodes[ridge, 13] - (1.0 - np.cos(np.pi / 4))).max() <= 32 * rc.EPS
    assert np.abs(nodes[off, 13]).max() <= 32 * rc.EPS
    fs.close()


# ------------------------------------------------------------------ 2. the slice walk (child processes)

WORKER = os.path.join(ROOT, "tests", "helpers", "recovery_worker.py")
CHILD_TIMEOUT = 240


def test_more_slices_than_workgroups_give_the_bits_of_the_default_grid(tmp_path):
    """336 nodes in 11 slices under FEMSHELL_SLICE_GRID=8: workgroups take a second slice, and every bit is that of the default
    grid.  One child per setting, one after another; a child that does not exit 0 ends the test."""
    from tests.helpers.recovery_worker import problem
    got = {}
    for grid in ("default", "8"):
        env = dict(os.environ)
        env.pop("FEMSHELL_SLICE_GRID", None)
        if grid != "default":
            env["FEMSHELL_SLICE_GRID"] = grid
        out = str(tmp_path / ("out_%s.npz" % grid))
        r = subprocess.run([sys.executable, WORKER, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT)
        assert r.returncode == 0, "grid %s failed:\n%s" % (grid, r.stdout.decode(errors="replace")[-1500:])
        got[grid] = dict(np.load(out))
    base, capped = got["default"], got["8"]
    xyz, tri, u = problem()
    assert len(xyz) > 256 and int(base["slices"]) == 11 and (int(capped["slices"]) + 7) // 8 > 8 // 8
    assert int(base["same"]) == 1 and int(capped["same"]) == 1
    np.testing.assert_array_equal(capped["nodes"], base["nodes"])
    np.testing.assert_array_equal(capped["elems"], base["elems"])
    _held("panel_20x15", rc.Recovery(xyz, tri, None, u), base["nodes"], base["elems"])


# ------------------------------------------------------------------ 3. other context states

def test_null_form_after_a_solve_with_prescribed_values():
    """u = None: the last solution, prescribed part included -- the bits of the explicit form, within the bounds of the reference
    on the same u, and not those of the homogeneous part"""
    xyz, tri, mask, ubar, _ = pr.cantilever()
    fs = _context(xyz, tri, None)
    fs.set_dirichlet(mask)
    fs.set_prescribed(ubar)
    u, info = fs.solve(rtol=1e-12, max_it=50000)
    assert info["converged"] == 1
    nodes, elems = fs.nodal_resultants()
    explicit = fs.nodal_resultants(u)
    assert np.array_equal(nodes, explicit[0]) and np.array_equal(elems, explicit[1])
    ref = rc.Recovery(xyz, tri, None, u)
    _held("cantilever_prescribed", ref, nodes, elems)
    without = rc.Recovery(xyz, tri, None, np.where(pr.fixed_dofs(mask).reshape(-1, 6), 0.0, u))
    assert max(ref.ratios(without.nodes, without.elems)) > 1.0
    fs.close()


def test_temperatures_in_force():
    """N_e, M_e are the rows element_resultants gives while temperatures are in force: the free thermal state has left them"""
    xyz, tri = pr.panel(lift=True)
    fs = _context(xyz, tri, None)
    fs.set_expansion(1.2e-5)
    tt, _ = th.random_temps(len(tri), 0)
    fs.set_thermal(tt, None)
    u = rs.random_u(len(xyz), seed=12) * 1e-3
    nodes, elems = fs.nodal_resultants(u)
    res, S = th.mesh_resultants(xyz, tri, None, u, tt, None, 1.2e-5)
    ref = rc.Recovery(xyz, tri, None, u, res_given=(res.astype(np.float64), S.astype(np.float64)))
    _held("lifted_panel_heated", ref, nodes, elems)
    cold = rc.Recovery(xyz, tri, None, u)
    assert max(ref.ratios(cold.nodes, cold.elems)) > 1.0
    fs.close()


def test_rows_are_the_callers_nodes_and_elements(monkeypatch):
    """under a renumbering, with a section of its own per element: node row i is the caller's node i, element row j the caller's
    element j -- the reference's element rows are pairwise different, so no permutation of them passes"""
    from tests.helpers import meshes
    monkeypatch.setenv("FEMSHELL_REORDER", "rcm")
    xyz, tri, quad = meshes.mixed_petals(24)
    ne = len(tri) + len(quad)
    table = np.stack([0.05 + 0.01 * np.arange(ne), 1e5 * (1.0 + 0.37 * np.arange(ne)), 0.02 * (1.0 + 0.11 * np.arange(ne))], axis=1)
    sec = (table, np.arange(len(tri), dtype=np.int32), len(tri) + np.arange(len(quad), dtype=np.int32))
    fs = _context(xyz, tri, quad, sec)
    u = rs.random_u(len(xyz), seed=9)
    nodes, elems = fs.nodal_resultants(u)
    ref = rc.Recovery(xyz, tri, quad, u, sec=sec)
    _held("mixed_petals24_own_sections_rcm", ref, nodes, elems)
    assert len(np.unique(ref.elems[:, 0])) == ne
    fs.close()


# ------------------------------------------------------------------ 4. the context stays as it was

def test_the_call_leaves_the_context_untouched():
    """element_resultants, the solution in HBM and a repeated solve give the same bits before and after the call"""
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    loads = np.zeros((n, 6))
    loads[:, :3] = np.random.default_rng(3).normal(size=(n, 3)) * [5.0, 5.0, 0.5]
    fs = _context(xyz, tri, None)
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    u0, info = fs.solve(rtol=1e-12, max_it=50000)
    assert info["converged"] == 1
    before = fs.element_resultants()
    other = rs.random_u(n, seed=21)
    fs.nodal_resultants(other)
    fs.nodal_resultants()
    assert np.array_equal(fs.get_solution(), u0)
    assert np.array_equal(fs.element_resultants(), before)
    u1, info1 = fs.solve(rtol=1e-12, max_it=50000)
    assert np.array_equal(u1, u0) and info1["iterations"] == info["iterations"]
    fs.close()


# ------------------------------------------------------------------ 5. refusals

def test_refusals_leave_the_context_usable():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    u = rs.random_u(n)
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    with pytest.raises(pkg.FemShellError) as e:
        fs.nodal_resultants(np.zeros(0))
    assert e.value.code == -1 and "no mesh" in str(e.value)
    fs.set_mesh(xyz, tri)
    with pytest.raises(pkg.FemShellError) as e:
        fs.nodal_resultants()
    assert e.value.code == -1 and "no solve has run" in str(e.value)
    good = fs.nodal_resultants(u)
    uc = np.ascontiguousarray(u)
    assert fs._L.femshell_nodal_resultants(fs._h, uc.ctypes.data_as(fs._L.femshell_nodal_resultants.argtypes[1]), None, None) == -1  # both outputs null
    assert b"femshell_nodal_resultants: null argument" in fs._L.femshell_last_error()
    bad = u.copy()
    bad[5, 2] = np.nan
    with pytest.raises(pkg.FemShellError) as e:
        fs.nodal_resultants(bad)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    fs.set_dirichlet(mask)
    fs.set_density(7.8e-9)
    fs.dynamics_begin(1e-3)
    with pytest.raises(pkg.FemShellError) as e:
        fs.nodal_resultants(u)
    assert e.value.code == -1 and "dynamics" in str(e.value)
    fs.dynamics_end()
    again = fs.nodal_resultants(u)
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    # a degenerate element is reported by its number in the caller's list
    flat_xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=np.float64)
    other = pkg.FemShell(rs.NU, rs.E, rs.T)
    other.set_mesh(flat_xyz, np.array([[0, 1, 3], [1, 2, 3], [0, 1, 2]], np.int32))
    with pytest.raises(pkg.FemShellError) as e:
        other.nodal_resultants(rs.random_u(4))
    assert e.value.code == -4 and "triangle 2" in str(e.value)
    # a row partition
    part = pkg.FemShell(rs.NU, rs.E, rs.T, rank=0, world_size=2)
    with pytest.raises(pkg.FemShellError) as e:
        part.nodal_resultants(np.zeros(0))
    assert e.value.code == -7 and "single-rank" in str(e.value)
    fs.close()


# ------------------------------------------------------------------ 6. timing entries

@pytest.mark.parametrize("with_sections", [False, True])
def test_time_kernel_runs_both_kernels_and_returns_the_byte_models(with_sections):
    from tests.helpers import meshes, sections
    xyz, tri, quad = meshes.mixed_petals(24)
    sec = (sections.THREE, np.arange(len(tri), dtype=np.int32) % 3, np.arange(len(quad), dtype=np.int32) % 3) if with_sections else None
    fs = _context(xyz, tri, quad, sec)
    n, ne = len(xyz), len(tri) + len(quad)
    ms, nbytes = fs.time_kernel(pkg.KERNEL_NODAL_RECOVERY, reps=3)
    assert ms > 0.0
    assert nbytes == (16 + 4 + 96) * el.listed_elements(n, tri, quad) + 24 * n + 112 * 32 * ((n + 31) // 32)
    ms, nbytes = fs.time_kernel(pkg.KERNEL_RECOVERY_ERROR, reps=3)
    assert ms > 0.0
    assert nbytes == 12 * len(tri) + 16 * len(quad) + (96 + 16) * ne + (24 + 96) * n + (4 * ne if with_sections else 0)
    # the hook leaves the context as it was
    u = rs.random_u(n)
    nodes, elems = fs.nodal_resultants(u)
    _held("mixed_petals24_after_timing", rc.Recovery(xyz, tri, quad, u, sec=sec), nodes, elems)
    fs.close()
