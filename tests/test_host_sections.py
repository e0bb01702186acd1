"""Shell sections in the host tools: element tags of a Gmsh mesh (ShellMesh::elem_tag), the FEM-shell twin's -sections /
-section_ids options, the "section" cell array of its VTK file.  CPU: reader and parsers; GPU: the twin against the binding."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built

HOST = os.path.join(ROOT, "fem-shell_amd", "host")
NX, NY = 8, 5
TAG_LEFT, TAG_RIGHT = 7, 9
SECTIONS = {TAG_RIGHT: (0.25, 7.0e4, 0.1)}   # listed in the sections file; TAG_LEFT takes the command line's material
CMDLINE = (0.3, 2.0e5, 0.05)


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "meshConvert")


def plate():
    """curved plate of 2 * NX * NY triangles, two physical surfaces (left / right half), the edge x = 0 clamped"""
    xs, ys = np.meshgrid(np.arange(NX + 1) * 0.5, np.arange(NY + 1) * 0.4, indexing="xy")
    xyz = np.stack([xs.ravel(), ys.ravel(), 0.2 * np.sin(0.8 * xs.ravel())], axis=1)
    tri, tag = [], []
    for j in range(NY):
        for i in range(NX):
            n = j * (NX + 1) + i
            for t in ([n, n + 1, n + NX + 1], [n + 1, n + NX + 2, n + NX + 1]):
                tri.append(t)
                tag.append(TAG_LEFT if i < NX // 2 else TAG_RIGHT)
    clamped = np.flatnonzero(xs.ravel() == 0.0)
    loads = np.zeros((len(xyz), 6))
    loads[:, 2] = -1.0
    loads[:, 0] = 0.5
    return xyz, np.array(tri, np.int32), np.array(tag, np.int32), clamped, loads


def write_plate(tmp_path):
    xyz, tri, tag, clamped, loads = plate()
    lines = ["$MeshFormat", "2.2 0 8", "$EndMeshFormat", "$Nodes", str(len(xyz))]
    lines += ["%d %r %r %r" % (n + 1, float(x), float(y), float(z)) for n, (x, y, z) in enumerate(xyz)]
    lines += ["$EndNodes", "$Elements", str(len(tri) + len(clamped))]
    k = 1
    for t, g in zip(tri, tag):
        lines.append("%d 2 2 %d %d %d %d %d" % (k, g, g, t[0] + 1, t[1] + 1, t[2] + 1))
        k += 1
    for n in clamped:  # point elements: boundary id 1 (all six dofs fixed) on the node
        lines.append("%d 15 2 1 0 %d" % (k, n + 1))
        k += 1
    lines += ["$EndElements", ""]
    msh = tmp_path / "plate.msh"
    msh.write_text("\n".join(lines))
    with open(str(tmp_path / "plate_f"), "w") as f:
        f.write("%d 1.0\n" % len(xyz))
        for row in loads:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")
    sec = tmp_path / "plate.sections"
    sec.write_text("# tag  nu  E  t\n\n%d %r %r %r   # the right half\n" % ((TAG_RIGHT,) + SECTIONS[TAG_RIGHT]))
    return str(msh), str(sec)


def read_pvtu(index):
    """the .pvtu index and its piece, both parsed as XML: (cell arrays of the piece by name, names the index announces)"""
    import xml.etree.ElementTree as ET

    root = ET.parse(index).getroot()  # (a malformed index does not parse)
    assert root.tag == "VTKFile" and root.find(".//PPoints/PDataArray") is not None
    piece = os.path.join(os.path.dirname(index), root.find(".//Piece").get("Source"))
    assert piece.endswith("_0.vtu") and os.path.exists(piece)
    announced = [a.get("Name") for a in root.findall(".//PCellData/PDataArray")]
    proot = ET.parse(piece).getroot()
    cells = {a.get("Name"): np.array(a.text.split(), dtype=np.int64) for a in proot.findall(".//CellData/DataArray")}
    assert int(proot.find(".//Piece").get("NumberOfCells")) == len(proot.find(".//Cells/DataArray[@Name='types']").text.split())
    assert len(proot.findall(".//PointData/DataArray")) == 6 and len(root.findall(".//PPointData/PDataArray")) == 6
    return cells, announced


def test_gmsh_tags_round_trip_into_the_vtk_xml_files(tools, tmp_path):
    """the physical entities of a Gmsh mesh come back as the cell array "section" of the .pvtu / _0.vtu pair the coupled
    program writes (write_pvtu with sections in use, through meshConvert): index and piece are well-formed XML, the index
    announces the array and still names its piece"""
    _, conv = tools
    msh, _ = write_plate(tmp_path)
    out = str(tmp_path / "plate.pvtu")
    subprocess.check_call([conv, msh, out])
    cells, announced = read_pvtu(out)
    assert announced == ["section"]
    np.testing.assert_array_equal(cells["section"], plate()[2])
    # meshes without tags: zeros
    xda = str(tmp_path / "plate.xda")
    subprocess.check_call([conv, msh, xda])
    subprocess.check_call([conv, xda, str(tmp_path / "untagged.pvtu")])
    cells, _ = read_pvtu(str(tmp_path / "untagged.pvtu"))
    np.testing.assert_array_equal(cells["section"], np.zeros(2 * NX * NY, np.int64))


def test_sections_file_parser(tools, tmp_path):
    """comments and blank lines are accepted; a malformed line is refused with its line number -- before the program
    needs a GPU"""
    fem, _ = tools
    msh, sec = write_plate(tmp_path)
    base = [fem, "-nu", "0.3", "-e", "2e5", "-t", "0.05", "-mesh", msh]
    r = subprocess.run(base + ["-sections", sec], capture_output=True, text=True)
    assert "expected 'tag nu E t'" not in r.stderr and "n_elem()=80" in r.stdout
    bad = tmp_path / "bad.sections"
    bad.write_text("# two good lines, then one without a thickness\n7 0.3 1e5 0.1\n\n9 0.25 7e4\n")
    r = subprocess.run(base + ["-sections", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 4" in r.stderr and "expected 'tag nu E t'" in r.stderr
    bad.write_text("7 0.3 1e5 0.1\nseven 0.3 1e5 0.1\n")
    r = subprocess.run(base + ["-sections", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr
    bad.write_text("7 0.3 1e5 0.1\n7 0.3 1e5 0.2\n")
    r = subprocess.run(base + ["-sections", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "listed twice" in r.stderr
    ids = tmp_path / "short.ids"
    ids.write_text("7\n9\n")
    r = subprocess.run(base + ["-sections", sec, "-section_ids", str(ids)], capture_output=True, text=True)
    assert r.returncode != 0 and "2 ids for 80 elements" in r.stderr
    r = subprocess.run(base + ["-sections", str(tmp_path / "none")], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open" in r.stderr


def _cell_array(vtk_path, name):
    lines = open(vtk_path).read().splitlines()
    at = lines.index("SCALARS %s int 1" % name)
    n = int([l for l in lines[:at] if l.startswith("CELL_DATA")][-1].split()[1])
    return np.array(lines[at + 2:at + 2 + n], dtype=np.int64)


@pytest.mark.gpu
def test_twin_with_sections_equals_the_binding(tools, tmp_path):
    from tests.test_host_tools import _read_exodus

    pkg = ensure_built()
    fem, conv = tools
    msh, sec = write_plate(tmp_path)
    xyz, tri, tag, clamped, loads = plate()
    nu, E, t = CMDLINE
    fs = pkg.FemShell(nu, E, t)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(len(xyz), np.uint8)
    mask[clamped] = 0x3F
    fs.set_dirichlet(mask)
    fs.set_loads(loads)
    fs.set_sections([CMDLINE, SECTIONS[TAG_RIGHT]], (tag == TAG_RIGHT).astype(np.int32))
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=5000)
    assert info["converged"] == 1
    base = [fem, "-nu", repr(nu), "-e", repr(E), "-t", repr(t), "-mesh", msh]
    r = subprocess.run(base + ["-sections", sec, "-out", str(tmp_path / "S")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ex = _read_exodus(str(tmp_path / "S.e"))
    got = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(got - u) <= 1e-12 * np.linalg.norm(u)
    np.testing.assert_array_equal(_cell_array(str(tmp_path / "S.vtk"), "section"), tag)
    # the same through -section_ids on a mesh without tags
    xda = str(tmp_path / "plate2.xda")
    subprocess.check_call([conv, msh, xda])
    os.replace(str(tmp_path / "plate_f"), str(tmp_path / "plate2_f"))
    ids = tmp_path / "plate2.ids"
    ids.write_text("\n".join(str(int(g)) for g in tag) + "\n")
    r = subprocess.run([fem, "-nu", repr(nu), "-e", repr(E), "-t", repr(t), "-mesh", xda, "-sections", sec, "-section_ids", str(ids),
                        "-out", str(tmp_path / "T")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ex = _read_exodus(str(tmp_path / "T.e"))
    got = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(got - u) <= 1e-12 * np.linalg.norm(u)
    # without the options: no cell array, and the uniform material
    os.replace(str(tmp_path / "plate2_f"), str(tmp_path / "plate_f"))
    r = subprocess.run(base + ["-out", str(tmp_path / "U")], capture_output=True, text=True)
    assert r.returncode == 0 and "CELL_DATA" not in open(str(tmp_path / "U.vtk")).read()
    fs.set_sections(None)
    u0, _ = fs.solve(rtol=1e-12, max_it=5000)
    ex = _read_exodus(str(tmp_path / "U.e"))
    got = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(got - u0) <= 1e-12 * np.linalg.norm(u0)
    fs.close()


@pytest.mark.gpu
def test_coupled_twin_with_sections(tools, tmp_path):
    """FEM-shell-precice takes -sections / -section_ids through the same parser: a flap whose lower half is four times as
    thick bends less than the uniform one, every converged time step's .pvtu / _0.vtu pair parses as XML and carries the
    section array; without the options the files have no cell data"""
    from tests.helpers import meshes
    from tests.test_host_tools import CONFIG

    meshgen = os.path.join(HOST, "meshGen")
    coupled = os.path.join(HOST, "FEM-shell-precice")
    name = str(tmp_path / "flap")
    subprocess.check_call([meshgen, "t", "6", "40", "0", "0", "0.1", "1", "2,20,2,2", "1", "0", "1", "y", name])
    m = meshes.read_xda(name + ".xda")
    axis = int(np.argmax(np.ptp(m.xyz, axis=0)))  # along the flap
    mid = 0.5 * (m.xyz[:, axis].min() + m.xyz[:, axis].max())
    ids = np.where(m.xyz[m.tri][:, :, axis].mean(axis=1) < mid, 5, 0)
    (tmp_path / "flap.ids").write_text("\n".join(str(int(v)) for v in ids) + "\n")
    (tmp_path / "flap.sections").write_text("5 0.3 1e6 0.4  # the root half, four times as thick\n")
    cmd = [coupled, "-nu", "0.3", "-e", "1e6", "-t", "0.1", "-mesh", name + ".xda", "-config", CONFIG, "-dt", "0.01", "-axis", "y",
           "-steps", "2", "-fluid", "edge"]
    tips = {}
    for label, extra in (("uniform", []), ("sections", ["-sections", str(tmp_path / "flap.sections"), "-section_ids", str(tmp_path / "flap.ids")])):
        r = subprocess.run(cmd + extra + ["-out", str(tmp_path / label)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        tips[label] = [float(v) for v in re.findall(r"tip\[\d+\] node \d+ = (\S+)", r.stdout)]
        for t in range(2):
            cells, announced = read_pvtu(str(tmp_path / ("%s_%03d.pvtu" % (label, t))))
            if label == "sections":
                assert announced == ["section"]
                np.testing.assert_array_equal(cells["section"], ids)
            else:
                assert announced == [] and cells == {}
    assert len(tips["sections"]) == len(tips["uniform"]) >= 2
    assert 0.0 < abs(tips["sections"][-1]) < abs(tips["uniform"][-1])  # stiffer at the root: a smaller tip displacement
