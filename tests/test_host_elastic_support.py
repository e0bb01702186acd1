"""Elastic supports in the host programs: -foundation, -foundation_shear, the -element_foundation and -springs file readers,
-support_forces and the refused combinations (CPU: refused before the program needs a GPU), FEM-shell with all of them against the
binding (GPU).  The mesh is the 48-triangle strip of tests/test_host_prescribed.py."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built
from tests.test_host_prescribed import E, NU, T, cantilever, write_cantilever

HOST = os.path.join(ROOT, "fem-shell_amd", "host")
KN, KT = 250.0, 40.0


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")


def file_moduli(n_tri):
    """rows (kn, kt) of every third triangle, the others not listed"""
    rows = np.zeros((n_tri, 2))
    listed = np.arange(0, n_tri, 3)
    rows[listed] = np.random.default_rng(6).uniform(0.0, 1.0, (len(listed), 2)) * [600.0, 80.0]
    return listed, rows


def file_springs(n_nodes):
    """rows of every fifth node from node 2"""
    rows = np.zeros((n_nodes, 6))
    listed = np.arange(2, n_nodes, 5)
    rows[listed] = np.random.default_rng(7).uniform(0.0, 1.0, (len(listed), 6)) * [300.0, 200.0, 500.0, 4.0, 5.0, 6.0]
    return listed, rows


def write_files(tmp_path, n_tri, n_nodes):
    listed, rows = file_moduli(n_tri)
    text = "# elem  kn  kt\n\n"
    for e in listed[::-1]:  # (any order)
        text += "%d %r %r   # a comment\n" % (e, float(rows[e, 0]), float(rows[e, 1]))
    found = tmp_path / "strip.foundation"
    found.write_text(text)
    listed, rows = file_springs(n_nodes)
    text = "# node  kx ky kz  krx kry krz\n"
    for a in listed[::-1]:
        text += "%d %s\n" % (a, " ".join(repr(float(v)) for v in rows[a]))
    springs = tmp_path / "strip.springs"
    springs.write_text(text)
    return str(found), str(springs)


def test_support_flags_parser_and_refused_combinations(tools, tmp_path):
    """good flags are accepted up to the point where the program needs a GPU; a missing file, a malformed line and a negative value
    are refused while the command line is read, an index the mesh lacks or lists twice as soon as the mesh is read, -support_forces
    with -modes or -dt / -steps and every flag in the coupled program by exit status and message"""
    fem, coupled = tools
    msh, _ = write_cantilever(tmp_path)
    xyz, tri = cantilever()[:2]
    found, springs = write_files(tmp_path, len(tri), len(xyz))
    base = [fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh]
    good = (["-foundation", "250"], ["-foundation_shear", "40"], ["-element_foundation", found], ["-springs", springs],
            ["-foundation", "250", "-foundation_shear", "40", "-element_foundation", found, "-springs", springs, "-support_forces", "-reactions",
             "-stress", "-buckling", "2"],
            ["-foundation", "250", "-springs", springs, "-rho", "7.8e-9", "-modes", "3"],
            ["-foundation", "250", "-springs", springs, "-rho", "7.8e-9", "-dt", "1e-3", "-steps", "2"],
            ["-foundation", "0", "-support_forces"])
    for extra in good:
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert "Read command-line arguments.......OK" in r.stdout and "n_elem()=48" in r.stdout, (extra, r.stdout, r.stderr)
        for word in ("expected '", "out of range", "cannot open", "negative", "listed twice", ">= 0"):
            assert word not in r.stderr, (extra, r.stderr)
    for flag in ("-element_foundation", "-springs"):
        r = subprocess.run(base + [flag, str(tmp_path / "none")], capture_output=True, text=True)
        assert r.returncode != 0 and "cannot open" in r.stderr and "FAILED" in r.stdout and "n_elem()" not in r.stdout
    bad = tmp_path / "bad.foundation"
    for text, words in (("# a good line, then one without kt\n8 1.0 0.5\n\n17 1.0\n", ("bad.foundation: line 4", "expected 'elem kn kt'")),
                        ("8 1.0 0.5\neight 1.0 0.5\n", ("line 2", "expected 'elem kn kt'")),
                        ("8 1.0 0.5\n9 1.0 0.5 7\n", ("line 2", "expected 'elem kn kt'")),
                        ("8 1.0 0.5\n9 nan 0.5\n", ("line 2",)),  # (the stream does not read it as a number)
                        ("8 1.0 0.5\n9 1.0 -0.5\n", ("line 2", "negative")),
                        ("8 1.0 0.5\n-1 1.0 0.5\n", ("line 2", "out of range"))):
        bad.write_text(text)
        r = subprocess.run(base + ["-element_foundation", str(bad)], capture_output=True, text=True)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (text, r.stderr)
        assert "FAILED" in r.stdout and "n_elem()" not in r.stdout  # refused while the command line is read
    bad = tmp_path / "bad.springs"
    for text, words in (("3 1 2 3 4 5\n", ("bad.springs: line 1", "expected 'node kx ky kz krx kry krz'")),
                        ("3 1 2 3 4 5 6 7\n", ("line 1", "expected 'node")),
                        ("3 1 2 3 4 5 6\n4 1 2 -3 4 5 6\n", ("line 2", "negative")),
                        ("3 1 2 3 4 5 inf\n", ("line 1",))):
        bad.write_text(text)
        r = subprocess.run(base + ["-springs", str(bad)], capture_output=True, text=True)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (text, r.stderr)
        assert "FAILED" in r.stdout and "n_elem()" not in r.stdout
    for flag in ("-foundation", "-foundation_shear"):
        for value in ("much", "-3", "nan"):
            r = subprocess.run(base + [flag, value], capture_output=True, text=True)
            assert r.returncode != 0 and flag + " needs a finite number >= 0" in r.stderr and "FAILED" in r.stdout and "n_elem()" not in r.stdout
    # as soon as the mesh is read: an index the mesh lacks or lists twice
    bad = tmp_path / "late.foundation"
    bad.write_text("8 1.0 0.5\n\n48 1.0 0.5\n")  # the mesh has elements 0 .. 47
    r = subprocess.run(base + ["-element_foundation", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "late.foundation: line 3" in r.stderr and "out of range" in r.stderr and "48 elements" in r.stderr
    assert "n_elem()=48" in r.stdout and "Linear solver" not in r.stdout
    bad.write_text("8 1.0 0.5\n8 2.0 0.5\n")
    r = subprocess.run(base + ["-element_foundation", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "listed twice" in r.stderr and "Linear solver" not in r.stdout
    bad = tmp_path / "late.springs"
    bad.write_text("3 1 2 3 4 5 6\n%d 1 2 3 4 5 6\n" % len(xyz))
    r = subprocess.run(base + ["-springs", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "late.springs: line 2" in r.stderr and "out of range" in r.stderr and "%d nodes" % len(xyz) in r.stderr
    assert "Linear solver" not in r.stdout
    bad.write_text("3 1 2 3 4 5 6\n4 1 2 3 4 5 6\n3 1 2 3 4 5 6\n")
    r = subprocess.run(base + ["-springs", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 3" in r.stderr and "listed twice" in r.stderr and "Linear solver" not in r.stdout
    # -support_forces belongs to the static solve
    for extra in (["-rho", "7.8e-9", "-modes", "3"], ["-rho", "7.8e-9", "-dt", "1e-3", "-steps", "2"]):
        r = subprocess.run(base + ["-foundation", "250", "-support_forces"] + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "-support_forces belongs to the static solve" in r.stderr and "FAILED" in r.stdout and "n_elem()" not in r.stdout
    # the coupled program has none of them
    config = str(tmp_path / "no-config.xml")
    for extra in (["-foundation", "250"], ["-foundation_shear", "40"], ["-element_foundation", found], ["-springs", springs]):
        r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-dt", "0.01"] + extra,
                           capture_output=True, text=True)
        assert r.returncode != 0 and "options of the stand-alone program" in r.stderr and "FAILED" in r.stdout
    # (-support_forces meets the coupled program's own -dt in the shared reader first: refused there)
    r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-dt", "0.01", "-support_forces"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "-support_forces" in r.stderr and "FAILED" in r.stdout


@pytest.mark.gpu
def test_twin_with_uniform_moduli_and_both_files_equals_the_binding(tools, tmp_path):
    """uniform values and the file add up, the springs file gives the listed form; the solution and the support forces are the
    binding's"""
    from tests.test_host_tools import _read_exodus

    pkg = ensure_built()
    fem, _ = tools
    msh, _ = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, loads = cantilever()
    found, springs = write_files(tmp_path, len(tri), len(xyz))
    rows = file_moduli(len(tri))[1] + [KN, KT]
    n = len(xyz)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(n, np.uint8)
    mask[clamped] = 0x3F
    mask[tip] = 0x07
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.set_foundation(rows)
    fs.set_springs(file_springs(n)[1])
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=5000)
    assert info["converged"] == 1
    f = fs.support_forces()
    out = str(tmp_path / "H")
    run = subprocess.run([fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-foundation", repr(KN), "-foundation_shear", repr(KT),
                          "-element_foundation", found, "-springs", springs, "-support_forces", "-out", out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    ex = _read_exodus(out + ".e")
    got = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(got - u) <= 1e-12 * np.linalg.norm(u)
    # the supports carry weight in the solution: without them it is another one
    fs.set_foundation(None, None)
    fs.set_springs(None)
    u_bare, _ = fs.solve(rtol=1e-12, max_it=5000)
    assert np.linalg.norm(u - u_bare) > 1e-3 * np.linalg.norm(u)
    table = np.loadtxt(out + "_support.txt")
    assert table.shape == (n, 7) and np.array_equal(table[:, 0], np.arange(n))
    assert np.abs(table[:, 1:] - f).max() <= 1e-9 * np.abs(f).max()  # (two solves of the same system to rtol 1e-12, written with every digit)
    vtk = open(out + ".vtk").read()
    assert "support_f" in vtk and "support_m" in vtk
    fs.close()
