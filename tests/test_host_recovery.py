"""FEM-shell -stress_nodes against the binding: the two text files, the point arrays and the cell array of <out>.vtk."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built
from tests.test_gpu_resultants import HE, HNU, HT, W_TIP, cantilever, write_cantilever

pytestmark = pytest.mark.gpu

pkg = ensure_built()

HOST = os.path.join(ROOT, "fem-shell_amd", "host")


def _field(lines, name, comps, count):
    at = lines.index("%s %d %d double" % (name, comps, count))
    return np.array([[float(v) for v in l.split()] for l in lines[at + 1:at + 1 + count]])


def _scalars(lines, name, count):
    at = lines.index("SCALARS %s double 1" % name)
    assert lines[at + 1] == "LOOKUP_TABLE default"
    return np.array([float(v) for v in lines[at + 2:at + 2 + count]])


@pytest.mark.parametrize("with_stress", [False, True])
def test_fem_shell_stress_nodes_equals_the_binding(tmp_path, with_stress):
    """the curved strip of tests/test_gpu_resultants.py with prescribed tip values: every line of <out>_stress_nodes.txt and of
    <out>_error.txt is the binding's row of the same case to the printed digits, the header's sums and relative error are those of
    the lines, the VTK file holds the three point arrays and error_indicator = eta bit for bit -- with and without -stress"""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    fem = os.path.join(HOST, "FEM-shell")
    msh, pres = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, loads = cantilever()
    out = str(tmp_path / "S")
    run = subprocess.run([fem, "-nu", repr(HNU), "-e", repr(HE), "-t", repr(HT), "-mesh", msh, "-prescribed", pres, "-stress_nodes", "-out", out]
                         + (["-stress"] if with_stress else []), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    # the program's own solution (the ExodusII file holds its doubles) through the binding's explicit form, whose bits are those of
    # the NULL form the program calls
    from tests.test_host_tools import _read_exodus
    ex = _read_exodus(out + ".e")
    u_host = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.array_equal(u_host[tip, 2], np.full(len(tip), W_TIP))
    fs = pkg.FemShell(HNU, HE, HT)
    fs.set_mesh(xyz, tri)
    nodes, elems = fs.nodal_resultants(u_host)
    nn, ne = len(xyz), len(tri)
    text = open(out + "_stress_nodes.txt").read().splitlines()
    assert text[0].startswith("# node Nxx Nyy Nzz Nxy Nyz Nzx Mxx Myy Mzz Mxy Myz Mzx W fold")
    rows = [l.split() for l in text if not l.startswith("#")]
    assert [int(r[0]) for r in rows] == list(range(nn))
    for r, mine in zip(rows, nodes):
        assert r[1:] == [("%.15e" % v) for v in mine]
    text = open(out + "_error.txt").read().splitlines()
    head = [l for l in text if l.startswith("# sum_e2 ")]
    assert len(head) == 1
    words = head[0].split()
    assert words[1:6:2] == ["sum_e2", "sum_eta2", "relative_error"]
    se2, seta2, rel = (float(w) for w in words[2:7:2])
    rows = [l.split() for l in text if not l.startswith("#")]
    assert [int(r[0]) for r in rows] == list(range(ne))
    for r, mine in zip(rows, elems):
        assert r[1:] == [("%.15e" % v) for v in mine]
    printed = np.array([[float(r[1]), float(r[2])] for r in rows])
    assert abs(se2 - printed[:, 0].sum()) <= 1e-13 * se2 and abs(seta2 - printed[:, 1].sum()) <= 1e-13 * seta2
    assert abs(rel - np.sqrt(seta2 / (se2 + seta2))) <= 1e-14
    assert abs(rel - pkg.relative_error(elems)) <= 1e-14 and 0.0 < rel < 1.0
    assert ("relative error of the mesh = %.6e" % rel) in run.stdout
    lines = open(out + ".vtk").read().splitlines()
    assert np.array_equal(_field(lines, "membrane_force_nodes", 6, nn), nodes[:, 0:6])
    assert np.array_equal(_field(lines, "moment_nodes", 6, nn), nodes[:, 6:12])
    assert np.array_equal(_scalars(lines, "fold", nn), nodes[:, 13])
    assert "CELL_DATA %d" % ne in lines and lines.index("SCALARS fold double 1") < lines.index("CELL_DATA %d" % ne)
    assert np.array_equal(_scalars(lines, "error_indicator", ne), np.sqrt(elems[:, 1]))
    if with_stress:  # the arrays of -stress stay beside the new ones
        s = fs.element_resultants(u_host)
        assert np.array_equal(_scalars(lines, "von_mises_top", ne), s[:, 12])
        assert np.array_equal(_field(lines, "membrane_force", 6, ne), s[:, 0:6])
        assert os.path.exists(out + "_stress.txt")
    else:
        assert "SCALARS von_mises_top double 1" not in lines and not os.path.exists(out + "_stress.txt")
    fs.close()
