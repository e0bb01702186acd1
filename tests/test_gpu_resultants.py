"""Element stress resultants and surface stresses on the device (femshell_element_resultants, FemShell.element_resultants,
FEM-shell -stress) against tests/helpers/resultants.py, the reference tests/test_resultants_cpu.py pins."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import meshes, oracle, prescribed as pr, resultants as rs, sections
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

HOST = os.path.join(ROOT, "fem-shell_amd", "host")


def _context(xyz, tri, quad, sec=None, t=rs.T):
    fs = pkg.FemShell(rs.NU, rs.E, t)
    fs.set_mesh(xyz, tri, quad)
    if sec is not None:
        fs.set_sections(sec[0], sec[1], sec[2])
    return fs


# ------------------------------------------------------------------ 1. device against reference

@pytest.mark.parametrize("name", list(rs.device_meshes()))
def test_resultants_match_the_reference(name, monkeypatch):
    """per element and component of N and M: |out - ref| <= 1e-12 S, S = sum_j |(D B)_j| |d_j| carried through the rotation; the two
    von Mises values within 4e-12 (S_N / t + 6 S_M / t^2).  u random in (-1, 1); a Dirichlet set does not show; two calls give the
    same bits.  (tests/test_resultants_cpu.py holds the reference's own two evaluations to the same bound on every mesh here.)"""
    xyz, tri, quad, sec, env = rs.device_meshes()[name]()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fs = _context(xyz, tri, quad, sec)
    u = rs.random_u(len(xyz))
    out = fs.element_resultants(u)
    assert out.shape == ((0 if tri is None else len(tri)) + (0 if quad is None else len(quad)), 14)
    assert np.array_equal(out, fs.element_resultants(u))
    mask = np.zeros(len(xyz), np.uint8)
    mask[::3] = 0x15
    fs.set_dirichlet(mask)
    assert np.array_equal(out, fs.element_resultants(u))
    ref, S = rs.mesh_resultants(xyz, tri, quad, u, rs.NU, rs.E, rs.T, sec=sec)
    ratio = rs.bound_ratio(out, ref, S)
    print("element_resultants_vs_reference %-28s elements %5d  max |out - ref| / (1e-12 S) = %.3e" % (name, len(out), ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------ the clamped panel under nodal loads

def _loaded_panel():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    loads = np.zeros((n, 6))
    loads[:, :3] = np.random.default_rng(3).normal(size=(n, 3)) * [5.0, 5.0, 0.5]
    return xyz, tri, mask, loads


@functools.lru_cache(maxsize=None)
def _panel_reference():
    xyz, tri, mask, loads = _loaded_panel()
    return pr.Reference(xyz, tri, None, oracle.material(rs.NU, rs.E, rs.T), mask, loads, None)


@functools.lru_cache(maxsize=None)
def _panel_solved(pc):
    xyz, tri, mask, loads = _loaded_panel()
    fs = _context(xyz, tri, None)
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    if pc == "amg":
        fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-13, max_it=50000)
    assert info["converged"] == 1
    return fs, u


def test_resultants_of_a_solved_load_case_match_the_reference_on_the_same_u():
    """the device's own solution as input: smooth, with cancellation in every strain, where the random u has none"""
    xyz, tri, _, _ = _loaded_panel()
    fs, u = _panel_solved("jacobi")
    out = fs.element_resultants(u)
    ref, S = rs.mesh_resultants(xyz, tri, None, u, rs.NU, rs.E, rs.T)
    ratio = rs.bound_ratio(out, ref, S)
    print("element_resultants_vs_reference %-28s elements %5d  max |out - ref| / (1e-12 S) = %.3e" % ("lifted_panel_solved", len(out), ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("pc", ["jacobi", "amg"])
def test_physics_through_the_library(pc):
    """the library's solve and its resultants against the reference evaluated on the reference's solution (the oracle's assembly,
    refined LU).  The solves agree to 1e-10 ||u|| (the tolerance of tests/test_gpu_prescribed.py); an error of that size in every
    entry of u moves an element's values by at most 1e-10 ||u|| sum_j |(D B)_j|, the scale S formed with |d_j| = ||u||: the bound,
    beside the 1e-12 S of the element math."""
    xyz, tri, _, _ = _loaded_panel()
    ref = _panel_reference()
    fs, u = _panel_solved(pc)
    err = np.linalg.norm(u - ref.u) / np.linalg.norm(ref.u)
    assert err <= 1e-10
    out = fs.element_resultants()
    want, S = rs.mesh_resultants(xyz, tri, None, ref.u, rs.NU, rs.E, rs.T)
    _, S_u = rs.mesh_resultants(xyz, tri, None, ref.u, rs.NU, rs.E, rs.T, uniform_abs=np.linalg.norm(ref.u))
    ratio = (np.abs(out - want) / (1e-10 * S_u + rs.TINY * S)).max()
    print("physics %-6s: solve differs by %.2e, max |out - ref| / (1e-10 S(||u||) + 1e-12 S) = %.3e" % (pc, err, ratio))
    assert ratio <= 1.0
    assert np.abs(want[:, :12]).max() > 0.0 and want[:, 12:].min() > 0.0  # the case carries something


# ------------------------------------------------------------------ 2. reproducibility and forms

def test_null_form_gives_the_bits_of_the_explicit_form_with_prescribed_values():
    xyz, tri, mask, ubar, _ = pr.cantilever()
    fs = _context(xyz, tri, None)
    fs.set_dirichlet(mask)
    fs.set_prescribed(ubar)
    u, info = fs.solve(rtol=1e-12, max_it=50000)
    assert info["converged"] == 1
    s = fs.element_resultants()
    assert np.array_equal(s, fs.element_resultants())
    assert np.array_equal(s, fs.element_resultants(fs.get_solution()))
    assert np.array_equal(s, fs.element_resultants(u))
    ref, S = rs.mesh_resultants(xyz, tri, None, u, rs.NU, rs.E, rs.T)
    assert rs.bound_ratio(s, ref, S) <= 1.0  # the prescribed part is in: the tip moved by w = 0.01
    without, _ = rs.mesh_resultants(xyz, tri, None, np.where(pr.fixed_dofs(mask).reshape(-1, 6), 0.0, u), rs.NU, rs.E, rs.T)
    assert rs.bound_ratio(s, without, S) > 1.0


# ------------------------------------------------------------------ 3. order

@pytest.mark.parametrize("reorder", ["", "rcm", "morton"])
def test_rows_are_the_callers_elements(reorder, monkeypatch):
    """mixed mesh, one section per element, all different: row i is the caller's element i -- its triangles, then its
    quadrilaterals -- whatever numbering the library uses inside.  No two rows of the reference agree, so no permutation passes."""
    if reorder:
        monkeypatch.setenv("FEMSHELL_REORDER", reorder)
    xyz, tri, quad = meshes.mixed_petals(24)
    ne = len(tri) + len(quad)
    table = np.stack([0.05 + 0.01 * np.arange(ne), 1e5 * (1.0 + 0.37 * np.arange(ne)), 0.02 * (1.0 + 0.11 * np.arange(ne))], axis=1)
    sec = (table, np.arange(len(tri), dtype=np.int32), len(tri) + np.arange(len(quad), dtype=np.int32))
    fs = _context(xyz, tri, quad, sec)
    u = rs.random_u(len(xyz), seed=9)
    out = fs.element_resultants(u)
    ref, S = rs.mesh_resultants(xyz, tri, quad, u, rs.NU, rs.E, rs.T, sec=sec)
    assert rs.bound_ratio(out, ref, S) <= 1.0
    for i in range(ne):
        for j in range(ne):
            if i != j:
                assert rs.bound_ratio(ref[j], ref[i], S[i]) > 1.0, (i, j)


# ------------------------------------------------------------------ 5. refusals

def test_refusals_leave_the_context_usable():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    u = rs.random_u(n)
    fs = pkg.FemShell(rs.NU, rs.E, rs.T)
    with pytest.raises(pkg.FemShellError) as e:
        fs.element_resultants(np.zeros(0))
    assert e.value.code == -1 and "no mesh" in str(e.value)
    fs.set_mesh(xyz, tri)
    with pytest.raises(pkg.FemShellError) as e:
        fs.element_resultants()
    assert e.value.code == -1 and "no solve has run" in str(e.value)
    good = fs.element_resultants(u)
    assert fs._L.femshell_element_resultants(fs._h, None, None) == -1  # a null `out`
    assert b"null argument" in fs._L.femshell_last_error()
    assert np.array_equal(fs.element_resultants(u), good)
    bad = u.copy()
    bad[5, 2] = np.inf
    with pytest.raises(pkg.FemShellError) as e:
        fs.element_resultants(bad)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    assert np.array_equal(fs.element_resultants(u), good)
    # dynamics
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    fs.set_dirichlet(mask)
    fs.set_density(7.8e-9)
    fs.dynamics_begin(1e-3)
    with pytest.raises(pkg.FemShellError) as e:
        fs.element_resultants(u)
    assert e.value.code == -1 and "dynamics" in str(e.value)
    fs.dynamics_end()
    assert np.array_equal(fs.element_resultants(u), good)
    # a degenerate element (zero area, three different nodes) is reported by its number in the caller's list
    flat_xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=np.float64)
    other = pkg.FemShell(rs.NU, rs.E, rs.T)
    other.set_mesh(flat_xyz, np.array([[0, 1, 3], [1, 2, 3], [0, 1, 2]], np.int32))
    with pytest.raises(pkg.FemShellError) as e:
        other.element_resultants(rs.random_u(4))
    assert e.value.code == -4 and "triangle 2" in str(e.value)
    assert np.array_equal(fs.element_resultants(u), good)
    # a row partition
    part = pkg.FemShell(rs.NU, rs.E, rs.T, rank=0, world_size=2)
    with pytest.raises(pkg.FemShellError) as e:
        part.element_resultants(np.zeros(0))
    assert e.value.code == -7 and "single-rank" in str(e.value)


# ------------------------------------------------------------------ 6. timing entry

@pytest.mark.parametrize("with_sections", [False, True])
def test_time_kernel_runs_the_resultants_and_returns_the_byte_model(with_sections):
    xyz, tri, quad = meshes.mixed_petals(24)
    sec = (sections.THREE, np.arange(len(tri), dtype=np.int32) % 3, np.arange(len(quad), dtype=np.int32) % 3) if with_sections else None
    fs = _context(xyz, tri, quad, sec)
    ms, nbytes = fs.time_kernel(pkg.KERNEL_ELEMENT_RESULTANTS, reps=3)
    ne = len(tri) + len(quad)
    assert ms > 0.0
    assert nbytes == 12 * len(tri) + 16 * len(quad) + 112 * ne + (24 + 48) * len(xyz) + (4 * ne if with_sections else 0)
    # the hook leaves the context as it was
    u = rs.random_u(len(xyz))
    ref, S = rs.mesh_resultants(xyz, tri, quad, u, rs.NU, rs.E, rs.T, sec=sec)
    assert rs.bound_ratio(fs.element_resultants(u), ref, S) <= 1.0


# ------------------------------------------------------------------ 7. host program

NX, NY = 8, 3
HNU, HE, HT = 0.3, 2.0e5, 0.05
W_TIP = 0.02


def cantilever():
    """the curved strip of tests/test_host_prescribed.py: 2 * NX * NY triangles, the edge x = 0 clamped (boundary id 1), u, v, w
    fixed on the edge x = 4 (id 20)"""
    xs, ys = np.meshgrid(np.arange(NX + 1) * 0.5, np.arange(NY + 1) * 0.4, indexing="xy")
    xyz = np.stack([xs.ravel(), ys.ravel(), 0.1 * np.sin(0.8 * xs.ravel())], axis=1)
    tri = []
    for j in range(NY):
        for i in range(NX):
            n = j * (NX + 1) + i
            tri += [[n, n + 1, n + NX + 1], [n + 1, n + NX + 2, n + NX + 1]]
    clamped = np.flatnonzero(xs.ravel() == 0.0)
    tip = np.flatnonzero(xs.ravel() == xs.max())
    loads = np.zeros((len(xyz), 6))
    loads[:, 2] = -0.3
    loads[:, 1] = 0.7
    return xyz, np.array(tri, np.int32), clamped, tip, loads


def write_cantilever(tmp_path):
    xyz, tri, clamped, tip, loads = cantilever()
    lines = ["$MeshFormat", "2.2 0 8", "$EndMeshFormat", "$Nodes", str(len(xyz))]
    lines += ["%d %r %r %r" % (n + 1, float(x), float(y), float(z)) for n, (x, y, z) in enumerate(xyz)]
    lines += ["$EndNodes", "$Elements", str(len(tri) + len(clamped) + len(tip))]
    k = 1
    for t in tri:
        lines.append("%d 2 2 5 5 %d %d %d" % (k, t[0] + 1, t[1] + 1, t[2] + 1))
        k += 1
    for nodes, bid in ((clamped, 1), (tip, 20)):  # point elements: a boundary id on the node
        for n in nodes:
            lines.append("%d 15 2 %d 0 %d" % (k, bid, n + 1))
            k += 1
    lines += ["$EndElements", ""]
    msh = tmp_path / "strip.msh"
    msh.write_text("\n".join(lines))
    with open(str(tmp_path / "strip_f"), "w") as f:
        f.write("%d 1.0\n" % len(xyz))
        for row in loads:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    pres = tmp_path / "strip.prescribed"
    pres.write_text("# node  u v w  tx ty tz\n" + "".join("%d 0 0 %r 0 0 0\n" % (n, W_TIP) for n in tip))
    return str(msh), str(pres)


def test_fem_shell_stress_equals_the_binding(tmp_path):
    """FEM-shell -prescribed FILE -stress -reactions: every line of <out>_stress.txt is the binding's row of the same case to the
    printed digits, the VTK file holds the four cell arrays with one tuple per element, bit for bit"""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    fem = os.path.join(HOST, "FEM-shell")
    msh, pres = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, loads = cantilever()
    fs = pkg.FemShell(HNU, HE, HT)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(len(xyz), np.uint8)
    mask[clamped] = 0x3F
    mask[tip] = 0x07
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    ubar = np.zeros((len(tip), 6))
    ubar[:, 2] = W_TIP
    fs.set_prescribed(ubar, node_ids=tip)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=5000)
    assert info["converged"] == 1 and np.array_equal(u[tip, 2], np.full(len(tip), W_TIP))
    out = str(tmp_path / "S")
    run = subprocess.run([fem, "-nu", repr(HNU), "-e", repr(HE), "-t", repr(HT), "-mesh", msh, "-prescribed", pres, "-stress", "-reactions",
                          "-out", out],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    # the same case: the program's own solution, prescribed values included (the ExodusII file holds its doubles), through the
    # binding's explicit form, whose bits are those of the NULL form the program calls
    from tests.test_host_tools import _read_exodus
    ex = _read_exodus(out + ".e")
    u_host = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(u_host - u) <= 1e-10 * np.linalg.norm(u)
    s = fs.element_resultants(u_host)
    assert "Element resultants" in run.stdout
    text = open(out + "_stress.txt").read().splitlines()
    assert text[0].startswith("# element Nxx Nyy Nzz Nxy Nyz Nzx Mxx Myy Mzz Mxy Myz Mzx von_mises_top von_mises_bottom")
    rows = [l.split() for l in text if not l.startswith("#")]
    assert [int(r[0]) for r in rows] == list(range(len(tri)))
    for r, mine in zip(rows, s):
        assert r[1:] == [("%.15e" % v) for v in mine]
    lines = open(out + ".vtk").read().splitlines()
    ne = len(tri)
    assert "CELL_DATA %d" % ne in lines
    for name, col in (("von_mises_top", 12), ("von_mises_bottom", 13)):
        at = lines.index("SCALARS %s double 1" % name)
        assert lines[at + 1] == "LOOKUP_TABLE default"
        assert np.array_equal(np.array([float(v) for v in lines[at + 2:at + 2 + ne]]), s[:, col])
    for name, cols in (("membrane_force", slice(0, 6)), ("moment", slice(6, 12))):
        at = lines.index("%s 6 %d double" % (name, ne))
        arr = np.array([[float(v) for v in l.split()] for l in lines[at + 1:at + 1 + ne]])
        assert arr.shape == (ne, 6) and np.array_equal(arr, s[:, cols])
    assert "VECTORS reaction_f double" in lines  # together with -reactions
    fs.close()
