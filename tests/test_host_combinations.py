"""Load combinations in the host programs: the reader of -combinations FILE2 and its refusals through FEM-shell (CPU: refused before
the program needs a GPU), the reader under the sanitizers as a stand-alone program (CPU), and one FEM-shell -load_cases
-combinations run of three cases and four combinations against the binding (GPU).  The strip and its three cases are those of
tests/test_host_load_cases.py."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built
from tests.test_host_load_cases import write_cases
from tests.test_host_prescribed import E, NU, T, cantilever, write_cantilever

HOST = os.path.join(ROOT, "fem-shell_amd", "host")

FACTORS = np.array([[1.35, 1.5, 0.0], [1.0, 0.0, 0.9], [1.35, 1.5, -0.9], [0.0, -2.0, 0.25]])
GOOD = "# G Q W\n1.35 1.5 0   # ULS 1\n\n1.0 0.0 0.9\n1.35 1.5 -0.9\n0 -2 2.5e-1\n"


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")


def test_combinations_reader_refusals(tools, tmp_path):
    """a good file is accepted up to the point where the program needs a GPU; a wrong count on a line, a token that is no number
    or not finite, an empty file, 257 lines and -combinations without -load_cases are refused while the command line is read, by
    exit status and a message that names file and line; -stress stays refused; the coupled program refuses the option"""
    fem, coupled = tools
    msh, _ = write_cantilever(tmp_path)
    n = len(cantilever()[0])
    lst, _, _ = write_cases(tmp_path, n)
    base = [fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh]
    combos = tmp_path / "strip.combinations"
    combos.write_text(GOOD)
    r = subprocess.run(base + ["-load_cases", lst, "-combinations", str(combos)], capture_output=True, text=True)
    assert "Read command-line arguments.......OK" in r.stdout and "n_elem()=48" in r.stdout, (r.stdout, r.stderr)
    assert "strip.combinations" not in r.stderr

    def refused(args, *words):
        r = subprocess.run(base + args, capture_output=True, text=True)
        assert r.returncode != 0 and all(w in r.stderr for w in words), (args, r.stderr)
        assert "FAILED" in r.stdout and "n_elem()" not in r.stdout  # while the command line is read

    bad = tmp_path / "bad.combinations"
    for text, words in (("1 2 3\n1 2\n", ("bad.combinations: line 2", "expected 3 factors", "found 2")),
                        ("1 2 3 4\n", ("bad.combinations: line 1", "expected 3 factors", "found 4")),
                        ("1 2 3\n\n1 x 3\n", ("bad.combinations: line 3", "'x' is not a number")),
                        ("1 2 3.0.1\n", ("bad.combinations: line 1", "'3.0.1' is not a number")),
                        ("1 2 1e3q\n", ("bad.combinations: line 1", "'1e3q' is not a number")),
                        ("1 inf 3\n", ("bad.combinations: line 1", "not a finite number")),
                        ("1 2 nan\n", ("bad.combinations: line 1", "not a finite number")),
                        ("1 2 1e999\n", ("bad.combinations: line 1", "not a finite number")),
                        ("# nothing\n\n   \n", ("bad.combinations", "holds no combination")),
                        ("", ("bad.combinations", "holds no combination")),
                        ("1 2 3\n" * 256 + "# more\n1 2 3\n", ("bad.combinations: line 258", "more than 256 combinations"))):
        bad.write_text(text)
        refused(["-load_cases", lst, "-combinations", str(bad)], *words)
    bad.write_text("1 2 3\n" * 256)
    r = subprocess.run(base + ["-load_cases", lst, "-combinations", str(bad)], capture_output=True, text=True)
    assert "Read command-line arguments.......OK" in r.stdout  # 256 are allowed
    refused(["-load_cases", lst, "-combinations"], "-combinations needs a file")
    refused(["-load_cases", lst, "-combinations", str(tmp_path / "none")], "cannot open", "none")
    refused(["-combinations", str(combos)], "-combinations needs -load_cases")
    refused(["-load_cases", lst, "-combinations", str(combos), "-stress"], "-load_cases does not go together with", "-stress")
    config = str(tmp_path / "no-config.xml")
    r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-load_cases", lst,
                        "-combinations", str(combos)], capture_output=True, text=True)
    assert r.returncode != 0 and "-combinations" in r.stderr and "FAILED" in r.stdout
    help_text = subprocess.run([fem], capture_output=True, text=True)  # too few arguments: the usage text
    assert "-combinations:" in help_text.stdout + help_text.stderr


def test_reader_under_the_sanitizers(tmp_path):
    """`make san` in the host folder builds combinations_san -- read_combinations of load_cases.cpp with
    -fsanitize=address,undefined and a main of its own --; good and refused files run clean"""
    subprocess.check_call(["make", "-C", HOST, "-s", "san"])
    prog = os.path.join(HOST, "combinations_san")
    assert os.path.exists(os.path.join(HOST, "load_cases_san"))
    f = tmp_path / "c.combinations"
    f.write_text(GOOD)
    r = subprocess.run([prog, str(f), "3"], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "4 combinations of 3 cases"
    assert np.array_equal(np.array([[float(w) for w in l.split()] for l in lines[1:]]), FACTORS)
    for text, n_cases, word in (("1 2\n", 3, "expected 3 factors"), ("1 2 3 #" + "x" * 5000 + "\n" + "1 2 3\n" * 300, 3, "more than 256 combinations"),
                                ("1 -" + "9" * 400 + " 3\n", 3, "not a finite number"), ("1 2 0x\n", 3, "not a number"), ("#\n", 1, "holds no combination"),
                                ("", 32, "holds no combination"), (" ".join(["1e-400"] * 32) + "\n" + "7 " * 31 + "\n", 32, "found 31")):
        f.write_text(text)
        r = subprocess.run([prog, str(f), str(n_cases)], capture_output=True, text=True)
        assert r.returncode == 1 and word in r.stderr and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (text[:40], r.stderr)
    r = subprocess.run([prog, str(tmp_path / "none"), "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "cannot open" in r.stderr and "Sanitizer" not in r.stderr


@pytest.mark.gpu
def test_twin_with_three_cases_and_four_combinations_equals_the_binding(tools, tmp_path):
    """FEM-shell -load_cases -combinations with block-Jacobi on the strip: every line of <out>_envelope.txt is the binding's row of
    the same case to the printed digits, the twelve cell arrays of <out>_envelope.vtk hold the same values bit for bit"""
    pkg = ensure_built()
    fem, _ = tools
    msh, _ = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, _ = cantilever()
    n, ne = len(xyz), len(tri)
    lst, names, L = write_cases(tmp_path, n)
    combos = tmp_path / "strip.combinations"
    combos.write_text(GOOD)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(n, np.uint8)
    mask[clamped] = 0x3F
    mask[tip] = 0x07
    fs.set_dirichlet(mask)
    out = str(tmp_path / "H")
    run = subprocess.run([fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-pc_type", "bjacobi", "-load_cases", lst,
                          "-combinations", str(combos), "-out", out], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr)
    assert "Load combinations: 4 combinations of 3 cases" in run.stdout
    # the same case: the program's own displacements (its VTK files hold every digit) through the binding
    from tests.test_host_load_cases import _vtk_vectors
    u = np.array([np.hstack([_vtk_vectors("%s_case%d.vtk" % (out, k + 1), "displacement", n), _vtk_vectors("%s_case%d.vtk" % (out, k + 1), "rotation", n)])
                  for k in range(3)])
    env, gov, _ = fs.combination_envelope(u, FACTORS)
    text = open(out + "_envelope.txt").read().splitlines()
    assert text[0].startswith("# element von_mises_top_max von_mises_bottom_max N1_max N2_min M1_max M2_min governs_von_mises_top_max")
    rows = [l.split() for l in text if not l.startswith("#")]
    assert [int(r[0]) for r in rows] == list(range(ne))
    for r, e_row, g_row in zip(rows, env, gov):
        assert r[1:7] == [("%.15e" % v) for v in e_row]
        assert [int(w) for w in r[7:]] == list(g_row + 1)
    assert len(np.unique(gov)) > 1  # more than one combination governs somewhere
    lines = open(out + "_envelope.vtk").read().splitlines()
    assert "CELL_DATA %d" % ne in lines
    value_names = ["von_mises_top_max", "von_mises_bottom_max", "N1_max", "N2_min", "M1_max", "M2_min"]
    for k, name in enumerate(value_names):
        at = lines.index("SCALARS %s double 1" % name)
        assert lines[at + 1] == "LOOKUP_TABLE default"
        assert np.array_equal(np.array([float(v) for v in lines[at + 2:at + 2 + ne]]), env[:, k])
        at = lines.index("SCALARS governs_%s int 1" % name)
        assert [int(v) for v in lines[at + 2:at + 2 + ne]] == list(gov[:, k] + 1)
    # the undeformed mesh
    at = lines.index("POINTS %d double" % n)
    assert np.allclose(np.array([[float(w) for w in l.split()] for l in lines[at + 1:at + 1 + n]]), xyz, rtol=0, atol=1e-9)
    fs.close()
