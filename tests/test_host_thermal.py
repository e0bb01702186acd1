"""Thermal loads in the host programs: -alpha, -section_alpha, -temperature, -temperature_gradient, the -thermal file reader and
the refused combinations (CPU: refused before the program needs a GPU), FEM-shell -alpha -temperature -thermal -stress against the
binding (GPU).  The mesh is the 48-triangle strip of tests/test_host_prescribed.py."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built
from tests.test_host_prescribed import E, NU, T, cantilever, write_cantilever

HOST = os.path.join(ROOT, "fem-shell_amd", "host")
ALPHA, TM, TG = 1.2e-5, 40.0, -15.0


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")


def file_temps(n_tri):
    """rows (Tm, Tg) of every third triangle, the others not listed"""
    rows = np.zeros((n_tri, 2))
    listed = np.arange(0, n_tri, 3)
    rows[listed] = np.random.default_rng(6).uniform(-1.0, 1.0, (len(listed), 2)) * [60.0, 20.0]
    return listed, rows


def write_temps(tmp_path, n_tri):
    listed, rows = file_temps(n_tri)
    text = "# elem  Tm  Tg\n\n"
    for e in listed[::-1]:  # (any order)
        text += "%d %r %r   # a comment\n" % (e, float(rows[e, 0]), float(rows[e, 1]))
    path = tmp_path / "strip.thermal"
    path.write_text(text)
    return str(path)


def test_thermal_flags_parser_and_refused_combinations(tools, tmp_path):
    """good flags are accepted up to the point where the program needs a GPU; a missing file, a short line, an element the mesh does
    not have, temperatures without -alpha, -section_alpha without -sections or with a tag they do not list, and every flag with
    -modes are refused before, by exit status and message"""
    fem, coupled = tools
    msh, _ = write_cantilever(tmp_path)
    temps = write_temps(tmp_path, 48)
    sections = tmp_path / "strip.sections"
    sections.write_text("# tag nu E t\n3 0.25 7e4 0.1\n5 0.3 2e5 0.05\n")
    sec_alpha = tmp_path / "strip.section_alpha"
    sec_alpha.write_text("# tag alpha\n5 2.3e-5   # aluminium\n")
    base = [fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh]
    alpha = ["-alpha", repr(ALPHA)]
    good = (alpha, alpha + ["-temperature", "40"], alpha + ["-temperature_gradient", "-15"], alpha + ["-thermal", temps],
            alpha + ["-temperature", "40", "-temperature_gradient", "-15", "-thermal", temps, "-reactions", "-stress", "-buckling", "2"],
            alpha + ["-temperature", "40", "-sections", str(sections), "-section_alpha", str(sec_alpha)],
            alpha + ["-temperature", "40", "-pressure", "2.5"])
    for extra in good:
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert "Read command-line arguments.......OK" in r.stdout and "n_elem()=48" in r.stdout, (extra, r.stdout, r.stderr)
        for word in ("expected 'elem", "expected 'tag", "out of range", "cannot open", "-alpha", "not a tag"):
            assert word not in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + alpha + ["-thermal", str(tmp_path / "none")], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open" in r.stderr and "FAILED" in r.stdout
    bad = tmp_path / "bad.thermal"
    bad.write_text("# a good line, then one without Tg\n8 1.0 0.5\n\n17 1.0\n")
    r = subprocess.run(base + alpha + ["-thermal", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.thermal: line 4" in r.stderr and "expected 'elem Tm Tg'" in r.stderr
    assert "n_elem()" not in r.stdout  # refused while the command line is read
    bad.write_text("8 1.0 0.5\neight 1.0 0.5\n")
    r = subprocess.run(base + alpha + ["-thermal", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "n_elem()" not in r.stdout
    bad.write_text("8 1.0 0.5\n9 1.0 0.5 7\n")
    r = subprocess.run(base + alpha + ["-thermal", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "expected 'elem Tm Tg'" in r.stderr
    bad.write_text("8 1.0 0.5\n9 nan 0.5\n")
    r = subprocess.run(base + alpha + ["-thermal", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr
    bad.write_text("8 1.0 0.5\n-1 1.0 0.5\n")
    r = subprocess.run(base + alpha + ["-thermal", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "out of range" in r.stderr
    bad.write_text("8 1.0 0.5\n\n48 1.0 0.5\n")  # the mesh has elements 0 .. 47
    r = subprocess.run(base + alpha + ["-thermal", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.thermal: line 3" in r.stderr and "out of range" in r.stderr and "48 elements" in r.stderr
    assert "Linear solver" not in r.stdout
    bad.write_text("8 1.0 0.5\n8 2.0 0.5\n")
    r = subprocess.run(base + alpha + ["-thermal", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "listed twice" in r.stderr
    for flag in ("-alpha", "-temperature", "-temperature_gradient"):
        extra = (alpha if flag != "-alpha" else []) + [flag, "much"]
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and flag + " needs a finite number" in r.stderr and "FAILED" in r.stdout
    # temperatures need an expansion coefficient
    for extra in (["-temperature", "40"], ["-temperature_gradient", "-15"], ["-thermal", temps]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "need an expansion coefficient, -alpha" in r.stderr and "FAILED" in r.stdout and "n_elem()" not in r.stdout
    # -section_alpha: needs -sections, a well-formed file, tags that the -sections file lists
    r = subprocess.run(base + alpha + ["-temperature", "40", "-section_alpha", str(sec_alpha)], capture_output=True, text=True)
    assert r.returncode != 0 and "-section_alpha needs the sections" in r.stderr and "FAILED" in r.stdout
    bad_alpha = tmp_path / "bad.section_alpha"
    bad_alpha.write_text("5 2.3e-5\n3\n")
    r = subprocess.run(base + alpha + ["-temperature", "40", "-sections", str(sections), "-section_alpha", str(bad_alpha)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.section_alpha: line 2" in r.stderr and "expected 'tag alpha'" in r.stderr
    bad_alpha.write_text("5 2.3e-5\n5 1e-5\n")
    r = subprocess.run(base + alpha + ["-temperature", "40", "-sections", str(sections), "-section_alpha", str(bad_alpha)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "listed twice" in r.stderr
    bad_alpha.write_text("5 2.3e-5\n\n7 1e-5\n")
    r = subprocess.run(base + alpha + ["-temperature", "40", "-sections", str(sections), "-section_alpha", str(bad_alpha)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.section_alpha: line 3" in r.stderr and "not a tag of the -sections file" in r.stderr
    assert "Linear solver" not in r.stdout
    # not with -modes
    for extra in (alpha, alpha + ["-temperature", "40"], alpha + ["-temperature_gradient", "-15"], alpha + ["-thermal", temps]):
        r = subprocess.run(base + extra + ["-rho", "7.8e-9", "-modes", "3"], capture_output=True, text=True)
        assert r.returncode != 0 and "do not go together with -modes" in r.stderr and "FAILED" in r.stdout and "n_elem()" not in r.stdout
    # the coupled program has none of them
    config = str(tmp_path / "no-config.xml")
    for extra in (alpha, alpha + ["-temperature", "40"], alpha + ["-thermal", temps]):
        r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-dt", "0.01"] + extra,
                           capture_output=True, text=True)
        assert r.returncode != 0 and "options of the stand-alone program" in r.stderr and "FAILED" in r.stdout


@pytest.mark.gpu
def test_twin_with_uniform_values_and_a_thermal_file_equals_the_binding(tools, tmp_path):
    """uniform values and the file add up; the solution, and the stress file of the heated shell, are the binding's"""
    from tests.test_host_tools import _read_exodus

    pkg = ensure_built()
    fem, _ = tools
    msh, _ = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, loads = cantilever()
    path = write_temps(tmp_path, len(tri))
    _, rows = file_temps(len(tri))
    rows = rows + [TM, TG]
    n = len(xyz)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(n, np.uint8)
    mask[clamped] = 0x3F
    mask[tip] = 0x07
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.set_expansion(ALPHA)
    fs.set_thermal(rows)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=5000)
    assert info["converged"] == 1
    res = fs.element_resultants()
    out = str(tmp_path / "H")
    run = subprocess.run([fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-alpha", repr(ALPHA), "-temperature", repr(TM),
                          "-temperature_gradient", repr(TG), "-thermal", path, "-stress", "-out", out], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    ex = _read_exodus(out + ".e")
    got = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(got - u) <= 1e-12 * np.linalg.norm(u)
    # the temperatures carry weight in the solution: without them it is another one
    fs.set_thermal(None, None)
    u_cold, _ = fs.solve(rtol=1e-12, max_it=5000)
    assert np.linalg.norm(u - u_cold) > 1e-3 * np.linalg.norm(u)
    lines = [l.split() for l in open(out + "_stress.txt").read().splitlines() if l.strip() and not l.startswith("#")]
    stress = np.array([[float(v) for v in l[-14:]] for l in lines])
    assert stress.shape == res.shape
    assert np.abs(stress - res).max() <= 1e-9 * np.abs(res).max()  # (two solves of the same system to rtol 1e-12, written with every digit)
    fs.close()
