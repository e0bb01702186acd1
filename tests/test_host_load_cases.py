"""Load cases in the host programs: the -load_cases list reader and every refused combination (CPU: refused before the program
needs a GPU), the host-only parts under the sanitizers as a stand-alone program (CPU), and one FEM-shell -load_cases run of three
cases against the binding (GPU).  The mesh is the 48-triangle strip of tests/test_host_prescribed.py."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built
from tests.test_host_prescribed import E, NU, T, cantilever, write_cantilever

HOST = os.path.join(ROOT, "fem-shell_amd", "host")


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")


def case_loads(n):
    """three cases: the strip's own loads, a single-node load, seeded random loads"""
    L = np.zeros((3, n, 6))
    L[0] = cantilever()[4]
    L[1, n // 2, :3] = (0.0, 2.0, -5.0)
    L[2] = np.random.default_rng(21).uniform(-1.0, 1.0, (n, 6))
    return L


def write_cases(tmp_path, n):
    """the three force files (the last one in a folder of its own, by absolute path) and the list"""
    L = case_loads(n)
    (tmp_path / "far").mkdir(exist_ok=True)
    names = ["dead_f", "point_f", str(tmp_path / "far" / "random_f")]
    for name, rows in zip(names, L):
        with open(name if name.startswith("/") else str(tmp_path / name), "w") as f:
            f.write("%d 1.0\n" % n)
            for row in rows:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
    lst = tmp_path / "strip.cases"
    lst.write_text("# one force file per line\n\n%s   # the loads of the strip\n%s\n\n%s\n" % tuple(names))
    return str(lst), names, L


def test_load_cases_list_parser_and_refused_combinations(tools, tmp_path):
    """a good list is accepted up to the point where the program needs a GPU; a missing list, a missing listed file, a line of two
    words, an empty list, 33 cases and every option the list does not go together with are refused while the command line is read,
    by exit status and message; the coupled program refuses the option"""
    fem, coupled = tools
    msh, pres = write_cantilever(tmp_path)
    n = len(cantilever()[0])
    lst, names, _ = write_cases(tmp_path, n)
    base = [fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh]
    for extra in ([], ["-pc_type", "bjacobi"], ["-foundation", "250"], ["-out", str(tmp_path / "G")]):
        r = subprocess.run(base + ["-load_cases", lst] + extra, capture_output=True, text=True)
        assert "Read command-line arguments.......OK" in r.stdout and "n_elem()=48" in r.stdout, (extra, r.stdout, r.stderr)
        for word in ("cannot open", "expected one", "does not go together", "names no force file", "more than"):
            assert word not in r.stderr, (extra, r.stderr)

    def refused(args, *words):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (args, r.stderr)
        assert "FAILED" in r.stdout and "n_elem()" not in r.stdout  # while the command line is read
        return r

    refused(["-load_cases"], "-load_cases needs a file")
    refused(["-load_cases", str(tmp_path / "none.cases")], "cannot open", "none.cases")
    bad = tmp_path / "bad.cases"
    bad.write_text("dead_f\n\n# gone\nmissing_f\n")
    refused(["-load_cases", str(bad)], "bad.cases: line 4", "cannot open", "missing_f")
    bad.write_text("dead_f\ndead_f point_f\n")
    refused(["-load_cases", str(bad)], "bad.cases: line 2", "expected one force file per line")
    bad.write_text("# nothing but comments\n\n   \n")
    refused(["-load_cases", str(bad)], "bad.cases", "names no force file")
    bad.write_text("dead_f\n" * 32)
    r = subprocess.run(base + ["-load_cases", str(bad)], capture_output=True, text=True)
    assert "Read command-line arguments.......OK" in r.stdout  # 32 are allowed
    bad.write_text("dead_f\n" * 32 + "\npoint_f\n")
    refused(["-load_cases", str(bad)], "bad.cases: line 34", "more than 32 load cases")
    rho = ["-rho", "7.8e-9"]
    for extra, flag in ((rho + ["-modes", "3"], "-modes"), (["-buckling", "2"], "-buckling"), (rho + ["-dt", "1e-3", "-steps", "2"], "-dt -steps"),
                        (["-prescribed", pres], "-prescribed"), (["-reactions"], "-reactions"), (["-stress"], "-stress"),
                        (["-stress_nodes"], "-stress_nodes"), (["-foundation", "250", "-support_forces"], "-support_forces"),
                        (["-pressure", "3.0"], "-pressure"), (["-element_loads", pres], "-element_loads"),
                        (rho + ["-gravity", "0", "0", "-9.81"], "-gravity"), (["-alpha", "1e-5", "-temperature", "10"], "-alpha -temperature"),
                        (["-alpha", "1e-5", "-temperature_gradient", "10"], "-temperature_gradient"), (["-alpha", "1e-5", "-thermal", pres], "-thermal")):
        refused(["-load_cases", lst] + extra, "-load_cases does not go together with", flag)
    # the coupled program has no load cases, with and without its own -dt
    config = str(tmp_path / "no-config.xml")
    r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-load_cases", lst],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "-load_cases" in r.stderr and "FAILED" in r.stdout
    r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-dt", "0.01", "-load_cases", lst],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "-load_cases" in r.stderr and "FAILED" in r.stdout


def test_host_only_parts_under_the_sanitizers(tmp_path):
    """`make san` in the host folder: load_cases.cpp (list reader, option check) with -fsanitize=address,undefined as a stand-alone
    program; good and refused lists run clean"""
    subprocess.check_call(["make", "-C", HOST, "-s", "san"])
    prog = os.path.join(HOST, "load_cases_san")
    n = len(cantilever()[0])
    lst, names, _ = write_cases(tmp_path, n)
    r = subprocess.run([prog, lst, "-mesh", "x.msh", "-stress", "-load_cases", lst, "-thermal", "f"], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[:3] == ["dead_f -> %s" % (tmp_path / "dead_f"), "point_f -> %s" % (tmp_path / "point_f"), "%s -> %s" % (names[2], names[2])]
    assert lines[3] == "conflicts: -stress -thermal"
    bad = tmp_path / "bad.cases"
    for text, word in (("dead_f\nnone_f\n", "line 2: cannot open"), ("dead_f point_f\n", "expected one force file per line"), ("#\n", "names no force file"),
                       ("dead_f #" + "x" * 5000 + "\n" * 3 + "dead_f\n" * 40, "more than 32 load cases"), ("", "names no force file")):
        bad.write_text(text)
        r = subprocess.run([prog, str(bad)], capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (text[:40], r.stderr)
    r = subprocess.run([prog, str(tmp_path / "none")], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr and "Sanitizer" not in r.stderr


def _vtk_vectors(path, name, n):
    words = open(path).read().split("VECTORS %s double\n" % name)[1].split()[:3 * n]
    return np.array([float(w) for w in words]).reshape(n, 3)


@pytest.mark.gpu
def test_twin_with_three_cases_equals_the_binding(tools, tmp_path):
    """FEM-shell -load_cases with block-Jacobi on the strip: the displacements of <out>_case<k>.vtk and the lines of <out>_cases.txt
    are the binding's solve_cases to the digits they are written with"""
    pkg = ensure_built()
    fem, _ = tools
    msh, _ = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, _ = cantilever()
    n = len(xyz)
    lst, names, L = write_cases(tmp_path, n)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(n, np.uint8)
    mask[clamped] = 0x3F
    mask[tip] = 0x07
    fs.set_dirichlet(mask)
    u, cases, info = fs.solve_cases(L, rtol=1e-12, max_it=5000)
    assert all(c["converged"] == 1 for c in cases) and info["passes"] == 1
    out = str(tmp_path / "H")
    run = subprocess.run([fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-pc_type", "bjacobi", "-load_cases", lst, "-out", out],
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr)
    assert "Load cases: 3 cases in 1 pass" in run.stdout
    rows = [line.split() for line in open(out + "_cases.txt").read().splitlines()]
    assert len(rows) == 3
    for k in range(3):
        assert rows[k][:2] == [str(k + 1), names[k]]
        assert (int(rows[k][2]), int(rows[k][3])) == (cases[k]["iterations"], cases[k]["converged"])
        assert rows[k][4] == "%.15e" % cases[k]["rel_residual"]
        d, r = _vtk_vectors("%s_case%d.vtk" % (out, k + 1), "displacement", n), _vtk_vectors("%s_case%d.vtk" % (out, k + 1), "rotation", n)
        assert np.array_equal(np.hstack([d, r]), u[k])  # written with every digit
    fs.close()
