"""Element loads in the host programs: -pressure, the -element_loads file reader, -gravity and the refused combinations (CPU:
refused before the program needs a GPU), FEM-shell -pressure -element_loads -reactions against the binding (GPU).  The mesh is the
48-triangle strip of tests/test_host_prescribed.py."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built
from tests.test_host_prescribed import E, NU, T, cantilever, write_cantilever

HOST = os.path.join(ROOT, "fem-shell_amd", "host")
PRESSURE = 2.5


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")


def file_loads(n_tri):
    """rows (p, qx, qy, qz) of every third triangle, the others not listed"""
    rows = np.zeros((n_tri, 4))
    listed = np.arange(0, n_tri, 3)
    rows[listed] = np.random.default_rng(5).uniform(-1.0, 1.0, (len(listed), 4)) * [4.0, 0.3, 0.2, 1.5]
    return listed, rows


def write_loads(tmp_path, n_tri):
    listed, rows = file_loads(n_tri)
    text = "# elem  p  qx qy qz\n\n"
    for e in listed[::-1]:  # (any order)
        text += "%d %r %r %r %r   # a comment\n" % (e, *(float(v) for v in rows[e]))
    path = tmp_path / "strip.element_loads"
    path.write_text(text)
    return str(path)


def test_element_load_flags_parser_and_refused_combinations(tools, tmp_path):
    """good flags are accepted up to the point where the program needs a GPU; a missing file, a short line, an element the mesh does
    not have, -gravity without -rho and every flag with -modes are refused before, by exit status and message"""
    fem, coupled = tools
    msh, _ = write_cantilever(tmp_path)
    loads = write_loads(tmp_path, 48)
    base = [fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh]
    good = (["-element_loads", loads], ["-pressure", "2.5"], ["-rho", "7.8e-9", "-gravity", "0", "0", "-9810"],
            ["-pressure", "2.5", "-element_loads", loads, "-rho", "7.8e-9", "-gravity", "0", "0", "-9810", "-reactions", "-stress"])
    for extra in good:
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert "Read command-line arguments.......OK" in r.stdout and "n_elem()=48" in r.stdout, (extra, r.stdout, r.stderr)
        for word in ("expected 'elem", "out of range", "-gravity needs", "cannot open", "needs -dt"):
            assert word not in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["-element_loads", str(tmp_path / "none")], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open" in r.stderr and "FAILED" in r.stdout
    bad = tmp_path / "bad.element_loads"
    bad.write_text("# a good line, then one without qz\n8 1.0 0 0 0.5\n\n17 1.0 0 0\n")
    r = subprocess.run(base + ["-element_loads", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.element_loads: line 4" in r.stderr and "expected 'elem p qx qy qz'" in r.stderr
    assert "n_elem()" not in r.stdout  # refused while the command line is read
    bad.write_text("8 1.0 0 0 0.5\neight 1.0 0 0 0.5\n")
    r = subprocess.run(base + ["-element_loads", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "n_elem()" not in r.stdout
    bad.write_text("8 1.0 0 0 0.5\n-1 1.0 0 0 0.5\n")
    r = subprocess.run(base + ["-element_loads", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "out of range" in r.stderr
    bad.write_text("8 1.0 0 0 0.5\n\n48 1.0 0 0 0.5\n")  # the mesh has elements 0 .. 47
    r = subprocess.run(base + ["-element_loads", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.element_loads: line 3" in r.stderr and "out of range" in r.stderr and "48 elements" in r.stderr
    assert "Linear solver" not in r.stdout
    bad.write_text("8 1.0 0 0 0.5\n8 2.0 0 0 0.5\n")
    r = subprocess.run(base + ["-element_loads", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "listed twice" in r.stderr
    r = subprocess.run(base + ["-pressure", "much"], capture_output=True, text=True)
    assert r.returncode != 0 and "-pressure needs" in r.stderr and "FAILED" in r.stdout
    r = subprocess.run(base + ["-gravity", "0", "0", "-9810"], capture_output=True, text=True)
    assert r.returncode != 0 and "-gravity needs a density, -rho" in r.stderr and "FAILED" in r.stdout
    r = subprocess.run(base + ["-rho", "7.8e-9", "-gravity", "0", "-9810"], capture_output=True, text=True)
    assert r.returncode != 0 and "-gravity needs three" in r.stderr and "FAILED" in r.stdout
    # -rho alone still asks for the time stepping options: only -gravity makes it the density of a static solve
    r = subprocess.run(base + ["-rho", "7.8e-9"], capture_output=True, text=True)
    assert r.returncode != 0 and "-rho needs -dt and -steps" in r.stderr
    for extra in (["-pressure", "2.5"], ["-element_loads", loads], ["-gravity", "0", "0", "-9810"]):
        r = subprocess.run(base + extra + ["-rho", "7.8e-9", "-modes", "3"], capture_output=True, text=True)
        assert r.returncode != 0 and "do not go together with -modes" in r.stderr and "FAILED" in r.stdout and "n_elem()" not in r.stdout
    # the coupled program has none of them
    config = str(tmp_path / "no-config.xml")
    for extra in (["-pressure", "2.5"], ["-element_loads", loads], ["-rho", "7.8e-9", "-gravity", "0", "0", "-9810"]):
        r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-dt", "0.01"] + extra,
                           capture_output=True, text=True)
        assert r.returncode != 0 and "options of the stand-alone program" in r.stderr and "FAILED" in r.stdout


@pytest.mark.gpu
def test_twin_with_pressure_and_an_element_load_file_equals_the_binding(tools, tmp_path):
    from tests.helpers import oracle, prescribed as pr
    from tests.test_host_tools import _read_exodus

    pkg = ensure_built()
    fem, _ = tools
    msh, _ = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, loads = cantilever()
    path = write_loads(tmp_path, len(tri))
    _, rows = file_loads(len(tri))
    rows[:, 0] += PRESSURE
    n = len(xyz)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(n, np.uint8)
    mask[clamped] = 0x3F
    mask[tip] = 0x07
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.set_element_loads(rows)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=5000)
    assert info["converged"] == 1
    S = fs.element_load_vector()
    out = str(tmp_path / "P")
    run = subprocess.run([fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-pressure", repr(PRESSURE), "-element_loads", path,
                          "-reactions", "-out", out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    ex = _read_exodus(out + ".e")
    got = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(got - u) <= 1e-12 * np.linalg.norm(u)
    rows_r = [l.split() for l in open(out + "_reactions.txt").read().splitlines()]
    assert rows_r[-1][0] == "sum"
    total = np.array([float(v) for v in rows_r[-1][1:]])
    # the sum line balances the total applied force, nodal and element loads: the bound of tests/test_host_prescribed.py
    K_unc, _ = pr.matrices(xyz, tri, None, oracle.material(NU, E, T), mask)
    applied = loads[:, :3].sum(axis=0) + S[:, :3].sum(axis=0)
    assert np.abs(S[:, :3].sum(axis=0)).max() > 0.1 * np.abs(loads[:, :3].sum(axis=0)).max()  # the element loads carry weight
    assert np.abs(total[:3] + applied).max() <= 1e-12 * pr.row_scale(K_unc, u).sum()
    fs.close()
