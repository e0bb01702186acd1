"""Nodal stress recovery and the Zienkiewicz-Zhu indicator: the reference of tests/helpers/recovery.py pinned on the CPU, before any
device result is compared with it -- its quadratic form against the local compliance, the patch tests, the closed form of a
cantilever strip, the fold measure, its two evaluations on the meshes of the GPU tests -- and what the binding and FEM-shell
-stress_nodes must show without a GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import oracle, prescribed as pr, recovery as rc, resultants as rs
from tests.helpers.product import ROOT
from tests.test_resultants_cpu import BS, LS, PS, QUADS, THESIS_Y, TRIS, patch, place, rotated, rotation, strip

HOST = os.path.join(ROOT, "fem-shell_amd", "host")
NU, E, T = 0.3, 2.1e5, 0.37


# ------------------------------------------------------------------ 1. the quadratic form

@pytest.mark.parametrize("name", ["tri_in_space", "quad_warped", "tri_skewed", "quad_skewed"])
def test_quadratic_form_of_global_tensors_is_the_local_compliance(name):
    """cN(N, N) = N_loc^T (t Dm)^-1 N_loc and cM(M, M) = M_loc^T Dp^-1 M_loc to 1e-13 relative: the frame-free form of the global
    tensors is the plane-stress compliance of the local ones, on tilted and warped elements, for random u"""
    kind, key = name.split("_", 1)
    xyz = np.array((TRIS if kind == "tri" else QUADS)[key])
    tDm, Dp = rs.plane_material(NU, E, T)
    rng = np.random.default_rng(4)
    for _ in range(5):
        u = rng.uniform(-1.0, 1.0, (len(xyz), 6))
        out, _, N, M = rs.element_resultants(xyz, u, NU, E, T, with_local=True)
        cn, cm = rc.q_form(out[:6], out[:6], NU) / (E * T), 12.0 * rc.q_form(out[6:12], out[6:12], NU) / (E * T ** 3)
        cn_loc, cm_loc = N @ np.linalg.solve(tDm, N), M @ np.linalg.solve(Dp, M)
        assert abs(cn - cn_loc) <= 1e-13 * cn_loc and abs(cm - cm_loc) <= 1e-13 * cm_loc
        both = np.concatenate([out[:6], out[6:12]])
        assert abs(rc.c_form(both, both, NU, E, T) - (cn_loc + cm_loc)) <= 1e-13 * (cn_loc + cm_loc)


# ------------------------------------------------------------------ 2. patch tests

def _eta_floor(r):
    """the bound of eta^2 where the exact difference is zero: Q(delta), delta the node bound plus the element bound"""
    out = []
    for e, conn in enumerate(rc.elements_of(r.tri, r.quad)):
        nu, Ee, th = r.mats[e]
        a = rc.vector_area(r.xyz[conn])
        dl = [r.node_bound[i, :12] + rs.TINY * r.S[e, :12] for i in conn]
        w = rc.W_TRI if len(conn) == 3 else rc.W_QUAD
        out.append(np.sqrt(a @ a) * sum(w[i][j] * rc.c_form(dl[i], dl[j], nu, Ee, th) for i in range(len(conn)) for j in range(len(conn))))
    return np.array(out)


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_membrane_patch_is_recovered_at_every_node(kind):
    """constant strain eps0: every node's N* is t Dm eps0 (rotated) within the node bound (the convex combination of the elements'
    1e-12 S), its M* zero to 1e-12 |N| t, and eta^2 is zero to rounding: below Q(delta)"""
    plane, tri, quad = patch(kind)
    R = rotation()
    eps0 = np.array([1.1e-3, -0.4e-3, 0.7e-3])
    local = np.zeros((len(plane), 6))
    local[:, 0] = eps0[0] * plane[:, 0] + 0.5 * eps0[2] * plane[:, 1]
    local[:, 1] = eps0[1] * plane[:, 1] + 0.5 * eps0[2] * plane[:, 0]
    xyz, u = place(plane, local, R)
    r = rc.Recovery(xyz, tri, quad, u, NU, E, T)
    N0 = rs.plane_material(NU, E, T)[0] @ eps0
    ratio = (np.abs(r.nodes[:, :6] - rotated(N0, R)) / r.node_bound[:, :6]).max()
    floor = _eta_floor(r)
    print("membrane patch %-4s: |N* - N0| / bound = %.2e, |M*| / (|N| t) = %.2e, eta^2 / Q(delta) = %.2e"
          % (kind, ratio, np.abs(r.nodes[:, 6:12]).max() / (np.abs(N0).max() * T), (r.elems[:, 1] / floor).max()))
    assert ratio <= 1.0
    assert np.abs(r.nodes[:, 6:12]).max() <= 1e-12 * np.abs(N0).max() * T
    assert (r.elems[:, 1] <= floor).all()
    assert rc.relative_error(r.elems) <= 1e-10
    assert (r.elems[:, 0] > 0.0).all()


@pytest.mark.parametrize("kind", ["tri", "quad"])
def test_bending_patch_is_recovered_at_every_node(kind):
    """constant curvature: every node's M* is -Dp (a, b, c) (rotated) within the node bound, N* zero, eta^2 below Q(delta).  TRI3
    under the thesis form of Y only: Y as coded fails the bending patch"""
    plane, tri, quad = patch(kind)
    R = rotation()
    a, b, c = 0.7e-2, -0.4e-2, 0.3e-2
    x, y = plane[:, 0], plane[:, 1]
    local = np.zeros((len(plane), 6))
    local[:, 2] = 0.5 * (a * x * x + b * y * y + c * x * y)
    local[:, 3] = b * y + 0.5 * c * x
    local[:, 4] = -(a * x + 0.5 * c * y)
    xyz, u = place(plane, local, R)
    r = rc.Recovery(xyz, tri, quad, u, NU, E, T, flags=THESIS_Y)
    M0 = -rs.plane_material(NU, E, T)[1] @ np.array([a, b, c])
    ratio = (np.abs(r.nodes[:, 6:12] - rotated(M0, R)) / r.node_bound[:, 6:12]).max()
    floor = _eta_floor(r)
    print("bending patch %-4s: |M* - M0| / bound = %.2e, |N*| t / |M| = %.2e, eta^2 / Q(delta) = %.2e"
          % (kind, ratio, np.abs(r.nodes[:, :6]).max() * T / np.abs(M0).max(), (r.elems[:, 1] / floor).max()))
    assert ratio <= 1.0
    assert np.abs(r.nodes[:, :6]).max() * T <= 1e-12 * np.abs(M0).max()
    assert (r.elems[:, 1] <= floor).all()
    assert rc.relative_error(r.elems) <= 1e-10


# ------------------------------------------------------------------ 3. closed form on the cantilever strip

@functools.lru_cache(maxsize=None)
def _strip_recovery(nx, kind, flags=oracle.REF_DEFAULT):
    xyz, tri, quad = strip(nx, kind)
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    loads = np.zeros((n, 6))
    loads[pr.edge_nodes(xyz, 0, LS), 2] = PS * np.array([0.25, 0.5, 0.25])
    ref = pr.Reference(xyz, tri, quad, oracle.material(0.0, E, T, flags), mask, loads, None)
    return rc.Recovery(xyz, tri, quad, ref.u, 0.0, E, T, flags=flags)


@pytest.mark.parametrize("nx", [8, 16, 32])
def test_quad_strip_indicator_has_its_closed_form(nx):
    """Clamped strip (8 x 1, nu = 0, tip load P), nx columns of 2 rectangular DKQ cells: the elements carry the mean of the beam's
    linear moment, the recovered field is its interpolant but for the two ends, and the difference is linear across every element
    from -+P h / 2b (or from 0 to P h / 2b at the ends): eta^2 = A_e 12 / (E t^3) (P h / b)^2 / 12 for EVERY element, an
    effectivity of 1 (measured 1 +- 5.9e-10; asserted to 1e-8, the margin is the rounding of the reference solve on the finest
    strip), and the relative error of the mesh is 1 / (2 nx) (measured to 3.3e-13; asserted to 1e-9)."""
    r = _strip_recovery(nx, "quad")
    h = LS / nx
    exact = (h * BS / 2) * 12.0 / (E * T ** 3) * (PS * h / BS) ** 2 / 12.0
    eff = r.elems[:, 1] / exact
    rel = rc.relative_error(r.elems)
    print("quad strip %2d columns: effectivity in [%.12f, %.12f], |eff - 1| = %.2e, relative error %.15f (|. - 1/(2 nx)| = %.2e)"
          % (nx, eff.min(), eff.max(), np.abs(eff - 1).max(), rel, abs(rel - 0.5 / nx)))
    assert np.abs(eff - 1.0).max() <= 1e-8
    assert abs(rel - 0.5 / nx) <= 1e-9
    assert np.abs(r.nodes[:, 13]).max() <= 32 * rc.EPS  # flat


def test_triangle_strips_are_printed():
    """Specht's Y as coded gives effectivities from 0.7 to above 1000 on the 1 x 0.5 cells of the 8-column strip (the defect
    DESIGN.md 8d records): printed, not asserted"""
    for nx in (8, 16):
        for flags, label in ((oracle.REF_DEFAULT, "Y as coded"), (THESIS_Y, "thesis Y")):
            r = _strip_recovery(nx, "tri", flags)
            h = LS / nx
            exact = (h * BS / 4) * 12.0 / (E * T ** 3) * (PS * h / BS) ** 2 / 12.0
            eff = r.elems[:, 1] / exact
            print("tri strip %2d columns, %-10s: effectivity in [%.3g, %.3g], relative error %.4f (beam: %.4f)"
                  % (nx, label, eff.min(), eff.max(), rc.relative_error(r.elems), 0.5 / nx))
            assert np.isfinite(r.elems).all() and (r.elems >= 0.0).all()


# ------------------------------------------------------------------ 4. the fold measure

def test_fold_measure():
    """0 within 32 EPS on a flat patch (rotated in space); 1 - cos 45 deg on the ridge of two equal square panels at 90 degrees,
    0 away from it; 1 at the nodes of two coincident triangles of opposite orientation, whose M* is then zero"""
    plane, tri, _ = patch("tri")
    xyz, u = place(plane, np.random.default_rng(2).uniform(-1e-3, 1e-3, (len(plane), 6)), rotation())
    nodes, _ = rc.recover(xyz, tri, None, rs.mesh_resultants(xyz, tri, None, u, NU, E, T)[0])
    assert np.abs(nodes[:, 13]).max() <= 32 * rc.EPS
    xyz, quad, ridge = rc.folded_plate()
    res = np.ones((len(quad), 14))
    nodes, count = rc.recover(xyz, None, quad, res)
    off = np.setdiff1d(np.arange(len(xyz)), ridge)
    assert np.abs(nodes[ridge, 13] - (1.0 - np.cos(np.pi / 4))).max() <= 32 * rc.EPS
    assert np.abs(nodes[off, 13]).max() <= 32 * rc.EPS
    assert np.abs(nodes[:, :12] - 1.0).max() <= 16 * rc.EPS and count.max() == 4
    xyz = np.array([[0, 0, 0], [1, 0, 0.2], [0.3, 1, 0]], dtype=np.float64)
    tri = np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    res = np.zeros((2, 14))
    res[0, 6:12], res[1, 6:12] = 1.0, -1.0  # M changes sign with the node order
    nodes, _ = rc.recover(xyz, tri, None, res)
    assert np.array_equal(nodes[:, 13], np.ones(3)) and np.array_equal(nodes[:, 6:12], np.zeros((3, 6)))
    # no area: fourteen zeros
    nodes, _ = rc.recover(np.zeros((3, 3)), np.array([[0, 1, 2]], np.int32), None, np.ones((1, 14)))
    assert np.array_equal(nodes, np.zeros((3, 14)))


# ------------------------------------------------------------------ 5. the reference against itself, on the meshes of the GPU tests

@pytest.mark.parametrize("name", list(rc.device_meshes()))
def test_two_evaluations_of_the_reference_stay_within_the_bounds(name):
    """Before a mesh is relied on in tests/test_gpu_recovery.py: the FP64 evaluation and a second one in numpy's long double (the
    element rows as tests/test_resultants_cpu.py takes them a second time) differ by less than the bounds of
    tests/helpers/recovery.py in every entry, for the random u the device gets"""
    xyz, tri, quad, sec, _ = rc.device_meshes()[name]()
    u = rs.random_u(len(xyz))
    a = rc.Recovery(xyz, tri, quad, u, sec=sec)
    b = rc.Recovery(xyz, tri, quad, u, sec=sec, dtype=np.longdouble)
    ratios = a.ratios(b.nodes, b.elems)
    print("recovery FP64 vs extended %-28s nodes %5d  ratios to the bounds: tensors %.3e  W %.3e  fold %.3e  e2 %.3e  eta2 %.3e"
          % ((name, len(xyz)) + ratios))
    assert max(ratios) <= 1.0


# ------------------------------------------------------------------ 6. binding and host program

def test_binding_lists_the_entry_point_and_the_timing_entries():
    import importlib
    import re

    binding = importlib.import_module("fem-shell_amd.binding")
    pkg = importlib.import_module("fem-shell_amd")
    assert "femshell_nodal_resultants" in binding.SYMBOLS
    header = open(os.path.join(ROOT, "include", "femshell.h")).read()
    assert int(re.search(r"FEMSHELL_KERNEL_NODAL_RECOVERY = (\d+)", header).group(1)) == binding.KERNEL_NODAL_RECOVERY == pkg.KERNEL_NODAL_RECOVERY == 16
    assert int(re.search(r"FEMSHELL_KERNEL_RECOVERY_ERROR = (\d+)", header).group(1)) == binding.KERNEL_RECOVERY_ERROR == pkg.KERNEL_RECOVERY_ERROR == 17
    assert re.search(r"int femshell_nodal_resultants\(femshell_ctx \*ctx, const double \*u[^;]*, double \*nodes_out[^;]*,\s*double \*elems_out[^;]*\);", header)
    assert hasattr(binding.FemShell, "nodal_resultants")
    elems = np.array([[3.0, 1.0], [5.0, 0.0], [7.0, 0.0]])
    assert pkg.relative_error(elems) == rc.relative_error(elems) == 0.25
    assert pkg.relative_error(np.zeros((0, 2))) == 0.0


def test_stress_nodes_flag_is_refused_with_modes_and_time_stepping(tmp_path):
    """-stress_nodes belongs to the static solve: with -modes or -dt / -steps it is refused while the command line is read, before
    the program needs a GPU; the coupled program does not have the flag"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    fem, coupled = os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")
    msh = str(tmp_path / "none.msh")  # never opened: the refusal comes first
    base = ["-nu", "0.3", "-e", "2e5", "-t", "0.05", "-mesh", msh]
    for extra in (["-rho", "1e-9", "-modes", "3"], ["-rho", "1e-9", "-dt", "1e-3", "-steps", "2"]):
        r = subprocess.run([fem] + base + ["-stress_nodes"] + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "-stress_nodes belongs to the static solve" in r.stderr and "FAILED" in r.stdout
        assert "n_elem()" not in r.stdout
    r = subprocess.run([coupled] + base + ["-config", str(tmp_path / "no-config.xml"), "-dt", "0.01", "-stress_nodes"], capture_output=True, text=True)
    assert r.returncode != 0 and "-stress_nodes" in r.stderr and "FAILED" in r.stdout
    r = subprocess.run([fem, "-h"], capture_output=True, text=True)
    assert "-stress_nodes:" in r.stdout + r.stderr
