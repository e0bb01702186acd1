"""Host programs above the C ABI: meshGen twin, XDA/_f formats, FEM-shell command line.
CPU part: formats and error behaviour.  GPU part: the shipped examples through the CLI."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.helpers import meshes
from tests.helpers.product import ROOT

HOST = os.path.join(ROOT, "fem-shell_amd", "host")


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "meshGen")


@pytest.mark.parametrize("kind,ul_lr,dead,bc,loading", [("t", 1, "z", "0,0,0,0", 2), ("t", 0, "y", "2,20,2,2", 1),
                                                        ("q", 1, "z", "-1,1,0,-1", 2), ("t", 1, "x", "-1,-1,-1,21", 0)])
def test_meshgen_twin_matches_generator(tools, tmp_path, kind, ul_lr, dead, bc, loading):
    _, meshgen = tools
    name = str(tmp_path / "m")
    subprocess.check_call([meshgen, kind, "7", "5", "-1.5", "0", "2", "3", bc, "2.5", str(loading), str(ul_lr), dead, name])
    got = meshes.read_xda(name + ".xda")
    ids = tuple(int(v) for v in bc.split(","))
    want = meshes.structured(7, 5, -1.5, 0, 2, 3, kind=kind, ul_lr=bool(ul_lr), dead_axis=dead, bcids=ids,
                             factor=2.5, loading=loading)
    np.testing.assert_allclose(got.xyz, want.xyz, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(got.tri, want.tri)
    np.testing.assert_array_equal(got.quad, want.quad)
    assert got.bcs == want.bcs
    np.testing.assert_array_equal(got.dirichlet_mask(), want.dirichlet_mask())
    if loading:
        loads = meshes.read_forces(name + "_f", got.n_nodes)
        np.testing.assert_allclose(loads, want.loads, rtol=1e-5)  # the file keeps 6 significant digits
        assert np.all(loads[-1] == 0.0)  # meshGen writes n-1 rows (main_all.cpp:352,377)
    else:
        assert not os.path.exists(name + "_f")


def _meshgen_cases():
    with open(os.path.join(ROOT, "tests", "golden", "meshgen_ref", "CASES.txt")) as f:
        return [tuple(line.strip().split(": ", 1)) for line in f if line.strip()]


@pytest.mark.parametrize("name,args", _meshgen_cases())
def test_meshgen_twin_is_byte_identical_to_the_reference_tool(tools, tmp_path, name, args):
    # tests/golden/meshgen_ref/* were written by the reference's own meshGen (src/meshgen/main_all.cpp compiled as-is,
    # tools/gen_meshgen_fixtures.py); the twin must reproduce them byte for byte: connectivity, side-BC numbering,
    # the n-1 force rows and the six significant digits of coordinates and forces
    _, meshgen = tools
    out = str(tmp_path / name)
    subprocess.check_call([meshgen] + args.split() + [out], stdout=subprocess.DEVNULL)
    gold = os.path.join(ROOT, "tests", "golden", "meshgen_ref", name)
    for ext in (".xda", "_f"):
        if os.path.exists(gold + ext):
            with open(gold + ext, "rb") as a, open(out + ext, "rb") as b:
                assert a.read() == b.read(), name + ext
        else:
            assert not os.path.exists(out + ext)


def test_meshgen_twin_against_the_live_reference_tool(tools, tmp_path):
    # more argument sets than the fixtures above, including the 64x64 Test-G meshes: the reference meshGen's output files
    # are stored gzip-compressed under tests/golden/meshgen_ref/live/ (tools/gen_meshgen_fixtures.py) and the twin must
    # reproduce them byte for byte.  Where oracle/_ref/meshGen_ref has been built (`make -C oracle ref`), the live
    # reference tool must still write the stored bytes as well.
    import gzip

    live = os.path.join(ROOT, "tests", "golden", "meshgen_ref", "live")
    ref = os.path.join(ROOT, "oracle", "_ref", "meshGen_ref")
    with open(os.path.join(live, "CASES.txt")) as f:
        cases = [tuple(line.strip().split(": ", 1)) for line in f if line.strip()]
    assert len(cases) == 6
    _, meshgen = tools
    for name, args in cases:
        b = str(tmp_path / ("twin_" + name))
        subprocess.check_call([meshgen] + args.split() + [b], stdout=subprocess.DEVNULL)
        runs = [b]
        if os.path.exists(ref):
            a = str(tmp_path / ("ref_" + name))
            subprocess.check_call([ref] + args.split() + [a], stdout=subprocess.DEVNULL)
            runs.append(a)
        for ext in (".xda", "_f"):
            gold = os.path.join(live, name + ext + ".gz")
            for out in runs:
                assert os.path.exists(gold) == os.path.exists(out + ext), out + ext
            if os.path.exists(gold):
                with gzip.open(gold, "rb") as fg:
                    want = fg.read()
                for out in runs:
                    with open(out + ext, "rb") as fo:
                        assert fo.read() == want, args + ext


def test_libmesh_adaptor_compiles_against_the_test_only_mock(tmp_path):
    # host/libmesh_adaptor.hpp needs libMesh, which this image lacks; tests/helpers/libmesh_mock declares the handful
    # of libMesh classes it touches so that the header at least passes a compiler (-fsyntax-only).  A syntax check of
    # the binding, not a reference build: nothing is linked or run.
    tu = tmp_path / "adaptor_tu.cpp"
    tu.write_text('#define FEMSHELL_HAVE_LIBMESH 1\n#include "libmesh_adaptor.hpp"\n'
                  "void use(libMesh::EquationSystems &es, const libMesh::Parallel::Communicator &c) {\n"
                  '    femshell_libmesh::femshell_assemble_elasticity(es, "Elasticity");\n'
                  "    femshell_libmesh::FemShellLinearSolver s(c);\n"
                  # the non-converged branches of the solver hook: iteration limit and breakdown map to libMesh's reasons
                  "    femshell_libmesh::binding().last_info.converged = 0;\n"
                  "    bool its = s.get_converged_reason() == libMesh::DIVERGED_ITS;\n"
                  "    femshell_libmesh::binding().last_rc = FEMSHELL_ERR_BREAKDOWN;\n"
                  "    bool brk = s.get_converged_reason() == libMesh::DIVERGED_BREAKDOWN;\n"
                  "    s.print_converged_reason();\n    (void)its; (void)brk;\n}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "helpers", "libmesh_mock"), str(tu)])


def test_coupled_program_compiles_against_a_precice_declaration():
    # -DFEMSHELL_HAVE_PRECICE instantiates run_coupled_structure<precice::SolverInterface> (the reference's participant,
    # fem-shell_precice.cpp:50-52); preCICE is absent here, so tests/helpers/precice_mock declares the pre-1.0
    # SolverInterface methods the adapter calls.  Syntax check only, nothing is linked.
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-DFEMSHELL_HAVE_PRECICE",
                           "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "tests", "helpers", "precice_mock"),
                           os.path.join(HOST, "coupling.cpp")])


def test_cli_usage_and_missing_arguments(tools):
    fem, _ = tools
    r = subprocess.run([fem], capture_output=True, text=True)
    assert r.returncode != 0 and "Usage:" in r.stderr and "-nu -e -t -mesh [-out] [-d]" in r.stderr
    r = subprocess.run([fem, "-nu", "0.3", "-e", "1", "-mesh", "x.xda", "-d", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "Mesh thickness t not specified" in r.stderr
    r = subprocess.run([fem, "-nu", "0.3", "-e", "1", "-t", "1", "-mesh", "/nonexistent.xda"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open" in r.stderr


def parse_solution(stdout):
    rows = re.findall(r"u= (\S+), v= (\S+), w= (\S+), tx= (\S+), ty= (\S+), tz= (\S+)\]", stdout)
    return np.array(rows, dtype=np.float64)


@pytest.mark.gpu
def test_cli_reproduces_thesis_values(tools, tmp_path):
    fem, _ = tools
    mesh = os.path.join(meshes.MESH_DIR, "test_A_uv_t.xda")
    r = subprocess.run([fem, "-nu", "0.25", "-e", "30000", "-t", "1.0", "-mesh", mesh, "-out", str(tmp_path / "A")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    u = parse_solution(r.stdout)
    assert u.shape == (27, 6)
    assert u[22, 0] == pytest.approx(-0.0255988, abs=6e-8) and u[22, 1] == pytest.approx(0.0629549, abs=6e-8)
    assert u[26, 0] == pytest.approx(-0.0342621, abs=6e-8) and u[26, 1] == pytest.approx(0.1944070, abs=6e-7)
    assert os.path.exists(str(tmp_path / "A.vtk"))
    ex = _read_exodus(str(tmp_path / "A.e"))  # the reference's output file (fem-shell.cpp:1249): displaced mesh + u, v, w, tx, ty, tz
    m = meshes.load_example("test_A_uv_t")
    for v in range(6):
        np.testing.assert_allclose(ex["vals_nod_var%d" % (v + 1)][0], u[:, v], rtol=1e-5, atol=1e-12)  # stdout keeps 6 digits
    np.testing.assert_allclose(ex["coordx"], m.xyz[:, 0] + ex["vals_nod_var1"][0], rtol=0, atol=1e-15)
    assert "Times [s]" not in r.stderr
    mesh = os.path.join(meshes.MESH_DIR, "test_C_w_tA16.xda")
    r = subprocess.run([fem, "-nu", "0.3", "-e", "10.92", "-t", "1.0", "-mesh", mesh], capture_output=True, text=True,
                       env=dict(os.environ, FEMSHELL_TIMING="1"))
    assert r.returncode == 0, r.stderr
    assert parse_solution(r.stdout)[144, 2] == pytest.approx(1.15169, abs=6e-6)
    # FEMSHELL_TIMING=1: the phases of the run on stderr (the twin's short form of libMesh's performance log)
    line = [l for l in r.stderr.splitlines() if l.startswith("Times [s]:")]
    assert len(line) == 1 and "read mesh and loads" in line[0] and "symbolic phase" in line[0] and "total" in line[0], r.stderr


# ---------------------------------------------------------------- coupled program (preCICE adapter twin)

@pytest.fixture(scope="module")
def coupled_tool(tools):
    return os.path.join(HOST, "FEM-shell-precice")


TOWER = os.path.join(meshes.MESH_DIR, "bending_tower_tri_test.xda")
CONFIG = os.path.join(meshes.GOLDEN, "coupling", "inprocess_config.xml")


def test_coupled_cli_finds_the_43_interface_nodes(coupled_tool):
    # fluid_solver.cpp:45-47 and run_example.sh:53 hard-wire N = 43 for this mesh
    r = subprocess.run([coupled_tool, "-nu", "0.3", "-e", "1e6", "-t", "0.1", "-mesh", TOWER, "-config", CONFIG,
                        "-dt", "0.01", "-axis", "y"], capture_output=True, text=True)
    assert "coupling interface nodes = 43" in r.stdout
    m = meshes.read_xda(TOWER)
    assert len(m.interface_nodes()) == 43
    assert sorted(np.nonzero(m.dirichlet_mask())[0].tolist()) == [0, 1, 2]
    r = subprocess.run([coupled_tool, "-nu", "0.3", "-e", "1e6", "-t", "0.1", "-mesh", TOWER], capture_output=True, text=True)
    assert r.returncode != 0 and "preCICE configuration file not specified" in r.stderr  # PC:489
    r = subprocess.run([coupled_tool, "-nu", "0.3"], capture_output=True, text=True)
    assert r.returncode != 0 and "-config -dt [-axis]" in r.stderr


@pytest.mark.gpu
def test_coupled_run_reproduces_the_quasi_static_time_series(coupled_tool):
    from tests.helpers import oracle

    steps = 6
    r = subprocess.run([coupled_tool, "-nu", "0.3", "-e", "1e6", "-t", "0.1", "-mesh", TOWER, "-config", CONFIG, "-dt", "0.01",
                        "-axis", "y", "-steps", str(steps)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tips = [float(v) for v in re.findall(r"tip\[\d+\] node \d+ = (\S+)", r.stdout)]
    probe = int(re.search(r"tip\[0\] node (\d+)", r.stdout).group(1))
    assert len(tips) == steps
    assert r.stdout.count("Iterate") == steps  # two coupling iterations per time step
    # oracle: K u = F with the dummy fluid's forces f_x = 1 + sin(t/25.01) on its 21 left-edge vertices
    # (fluid_solver.cpp:95-118, 187-199), mapped nearest-neighbour (consistent) onto the structure's
    # interface nodes; in the shipped mesh the flagged sides put interior node 4 on the interface and
    # leave corner node 0 out, so this follows the file, not the geometry
    m = meshes.read_xda(TOWER)
    mat = oracle.material(0.3, 1e6, 0.1)
    fluid = np.array([[3.0, k * 0.1] for k in range(21)] + [[3.25, k * 0.1] for k in range(21)] + [[3.125, 2.0]])
    loads = np.zeros((m.n_nodes, 6))
    for n in m.interface_nodes():
        d2 = ((fluid - m.xyz[n, [0, 2]]) ** 2).sum(axis=1)
        if int(np.argmin(d2)) < 21:
            loads[n, 0] = 1.0
    assert int(loads[:, 0].sum()) == 21  # 20 left-edge nodes + the tie-broken interior node 4
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), loads)
    u_unit = oracle.direct_solve(r0, c0, v0, F0).reshape(-1, 6)
    want = [(1.0 + np.sin(t / 25.01)) * u_unit[probe, 0] for t in range(steps)]
    np.testing.assert_allclose(tips, want, rtol=1e-5)


@pytest.mark.gpu
def test_coupled_flap_config5_scaled(tools, coupled_tool, tmp_path):
    """BASELINE configs[4] scaled down: flap 0.1 x 1 in the x-z plane (dead axis y), bottom edge id 20, other
    edges id 2, E=1e6 nu=0.3 t=0.1, forces f_x = 1 + sin(t/25.01) on the left-edge interface nodes."""
    from tests.helpers import oracle

    _, meshgen = tools
    name = str(tmp_path / "flap")
    nx, nz = 10, 100
    subprocess.check_call([meshgen, "t", str(nx), str(nz), "0", "0", "0.1", "1", "2,20,2,2", "1", "0", "1", "y", name])
    steps = 4
    r = subprocess.run([coupled_tool, "-nu", "0.3", "-e", "1e6", "-t", "0.1", "-mesh", name + ".xda", "-config", CONFIG,
                        "-dt", "0.01", "-axis", "y", "-steps", str(steps), "-fluid", "edge"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    tips = [float(v) for v in re.findall(r"tip\[\d+\] node \d+ = (\S+)", r.stdout)]
    probe = int(re.search(r"tip\[0\] node (\d+)", r.stdout).group(1))
    m = meshes.read_xda(name + ".xda")
    ifn = m.interface_nodes()
    left = [n for n in ifn if abs(m.xyz[n, 0]) < 1e-12]
    assert len(left) == nz + 1
    loads = np.zeros((m.n_nodes, 6))
    loads[left, 0] = 1.0
    mat = oracle.material(0.3, 1e6, 0.1)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), loads)
    u_unit = oracle.refined_solve(r0, c0, v0, F0).reshape(-1, 6)
    want = [(1.0 + np.sin(t / 25.01)) * u_unit[probe, 0] for t in range(steps)]
    np.testing.assert_allclose(tips, want, rtol=1e-5)


@pytest.mark.gpu
def test_coupled_flap_config5_full_size(tools, coupled_tool, tmp_path):
    """BASELINE configs[4] at its own size (500 x 1000 squares = 1,000,000 tri3) through FEM-shell-precice, three time steps:
    K against the oracle's assembly over all blocks, the tip series = (1 + sin(t / 25.01)) x the unit-load displacement of a
    multigrid solve that is itself held to a manufactured solution below 1e-10, and ONE assembly for all coupling iterations
    (the reference re-assembles the constant K on every one, fem-shell_precice.cpp:271).  On one GPU: the 2-GPU form of the
    config needs hardware this box does not have (tests/test_host_tools.py::test_coupled_program_on_two_ranks runs the
    program row-partitioned over the test transport)."""
    from tests.helpers import fullsize

    _, meshgen = tools
    out = fullsize.coupled_flap_full_size(coupled_tool, meshgen, tmp_path, CONFIG, steps=3)
    assert out["returncode"] == 0, out
    assert out["triangles"] == 1000000 and out["left_edge_nodes"] == 1001
    assert out["time_steps"] == 3 and out["assemblies_of_K"] == 1, out
    mp = out["matrix_vs_oracle"]
    assert mp["same_pattern"] and mp["F_bitwise_equal"] and mp["max_entry_diff_over_max_entry"] <= 1e-12, mp
    assert out["unit_load_solve"]["converged"] == 1
    assert out["tip_series_max_rel_diff"] < 1e-5, out  # (the program prints six digits)
    run = out["manufactured"]["runs"][1]
    assert run["converged"] == 1 and run["rel_err_vs_manufactured"] < 1e-10, out["manufactured"]
    assert out["cg_iterations"] < 150 * out["coupling_iterations"], out
    assert out["program_phase_seconds"] and "coupling loop" in out["program_phase_seconds"], out


# ---------------------------------------------------------------- Gmsh input, PETSc-style options, several ranks

MSH_EXAMPLE = """$MeshFormat
2.2 0 8
$EndMeshFormat
$Nodes
4
1 -1.0 -1.0  0.0
2  1.0 -1.0  0.0
3 -1.0  1.0  0.0
4  1.0  1.0  0.0
$EndNodes
$Elements
7
1 2 2 0 0 1 2 3
2 2 2 0 0 2 4 3
3 15 2 0 0 1
4 15 2 0 0 2
5 15 2 1 0 3
6 15 2 1 0 4
7 1 2 20 0 2 4
$EndElements
"""


def test_gmsh_reader_follows_the_thesis_listing(tools, tmp_path):
    # doc/implementation.tex:103-124: two triangles are the mesh; the point elements put boundary id 0 on nodes 1, 2
    # and id 1 on nodes 3, 4 (first tag = boundary id); a 2-node line flags the element side it coincides with.
    # The program then fails at the GPU (none here) or runs; the reader's result shows in the mesh summary either way
    fem, _ = tools
    p = tmp_path / "two.msh"
    p.write_text(MSH_EXAMPLE)
    r = subprocess.run([fem, "-nu", "0.3", "-e", "1", "-t", "1", "-mesh", str(p)], capture_output=True, text=True)
    assert "n_nodes()=4" in r.stdout and "n_elem()=2" in r.stdout
    bad = tmp_path / "bad.msh"
    bad.write_text(MSH_EXAMPLE.replace("7 1 2 20 0 2 4", "7 1 2 20 0 1 4"))  # 1-4 is a diagonal, not a side
    r = subprocess.run([fem, "-nu", "0.3", "-e", "1", "-t", "1", "-mesh", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "not a side of any element" in r.stderr
    xdr = tmp_path / "m.xdr"
    xdr.write_bytes(b"\x00\x00\x00\x0elibMesh-0.7.0+\x00\x00")  # header only
    r = subprocess.run([fem, "-nu", "0.3", "-e", "1", "-t", "1", "-mesh", str(xdr)], capture_output=True, text=True)
    assert r.returncode != 0 and "truncated XDR" in r.stderr
    xdr.write_bytes(b"\x00\x00\x00\x0elibMesh-1.9.9+\x00\x00")
    r = subprocess.run([fem, "-nu", "0.3", "-e", "1", "-t", "1", "-mesh", str(xdr)], capture_output=True, text=True)
    assert r.returncode != 0 and "not one this reader knows" in r.stderr


def test_ascii_xda_reader_takes_what_a_stream_would_take(tools, tmp_path):
    """The XDA and force-file readers parse numbers straight out of the file buffer (host/mesh_io.cpp TextFile /
    NumberCursor): the same files a `stream >> value` reader accepts are accepted -- comments behind the numbers, CR LF line
    ends, plus signs, exponents, blank-separated columns -- and what it rejected is still rejected with the same words."""
    conv = os.path.join(HOST, "meshConvert")
    text = ("libMesh-0.7.0+\n2\t # number of elements\n4 # number of nodes\n.\nn/a\nn/a\nn/a\n2 # n_elem at level 0\n"
            "3 0 1 2 # a triangle\n3   1\t3 2\n"
            "+0.0 0.0 0\n1e0 0 0.\n.0 +1.5E+0 -0\n1 1.5 2.5e-1   # a node\n"
            "2\n0 0 1\n1 1 0\n")
    want_xyz = np.array([[0, 0, 0], [1, 0, 0], [0, 1.5, 0], [1, 1.5, 0.25]], dtype=float)
    for name, body in (("unix", text), ("dos", text.replace("\n", "\r\n"))):
        src = tmp_path / (name + ".xda")
        src.write_bytes(body.encode())
        out = str(tmp_path / (name + "_out.xda"))
        subprocess.check_call([conv, str(src), out])
        m = meshes.read_xda(out)
        np.testing.assert_array_equal(m.xyz, want_xyz)
        np.testing.assert_array_equal(m.tri, [[0, 1, 2], [1, 3, 2]])
        assert m.bcs == [(0, 0, 1), (1, 1, 0)]
    # a libMesh >= 0.9.2 file: blank lines behind the boundary-condition section (with and without a newline at the very end of
    # the file) are not a nodeset record; a real nodeset record behind them is read
    new_header = text.replace("libMesh-0.7.0+", "libMesh-0.9.2+")
    for name, tail, want_nodesets in (("blank_nl", "\n", 0), ("blank_nl_nl", "\n\n", 0), ("blank_no_nl", "\n  ", 0), ("none", "", 0),
                                      ("nodeset", "1 # nodesets\n3 21\n", 1), ("nodeset_blank", "1\n3 21\n\n", 1)):
        src = tmp_path / (name + ".xda")
        src.write_bytes((new_header + tail).encode())
        out = str(tmp_path / (name + "_out.xda"))
        subprocess.check_call([conv, str(src), out])
        m = meshes.read_xda(out)
        np.testing.assert_array_equal(m.tri, [[0, 1, 2], [1, 3, 2]])
        assert m.bcs == [(0, 0, 1), (1, 1, 0)]
        assert open(out).read().count("nodesets") == want_nodesets, name
    for broken, words in ((text.replace("3   1\t3 2", "3 1 x 2"), "bad element line 1"),
                          (text.replace("1e0 0 0.", "1e0 zero 0."), "bad node line 1"),
                          (text.replace("3 0 1 2 # a triangle", "4 0 1 2"), "unsupported element type 4"),
                          (text.replace("1 1 0\n", "1 7 0\n"), "names side 7"),
                          (text[:text.index("+0.0")], "truncated XDA file"),
                          (text.replace("2\t # number of elements", "two"), "bad element count")):
        src = tmp_path / "broken.xda"
        src.write_text(broken)
        r = subprocess.run([conv, str(src), str(tmp_path / "never.xda")], capture_output=True, text=True)
        assert r.returncode != 0 and words in r.stderr, (words, r.stderr)


def test_binary_xdr_round_trip(tools, tmp_path):
    """mesh.read() of the reference accepts *.xdr beside *.xda (fem-shell.cpp:35-37): the binary form of the same records
    (big-endian 32-bit integers / IEEE doubles, length-prefixed padded strings).  No libMesh here to write one, so the
    reader is held to the twin's writer: XDA -> XDR -> XDA is the identity on every shipped example, the byte layout of
    the header is checked by hand, and a Gmsh mesh with point boundary ids keeps them (nodeset record, 0.9.2+ header)."""
    conv = os.path.join(HOST, "meshConvert")
    for name in ("test_A_uv_t", "test_B_uv_q", "test_D_w_q_uni16", "test_G_mpi_64_q", "bending_tower_tri_test"):
        src = os.path.join(meshes.MESH_DIR, name + ".xda")
        xdr, back, direct = (str(tmp_path / (name + e)) for e in (".xdr", "_back.xda", "_direct.xda"))
        subprocess.check_call([conv, src, xdr])
        subprocess.check_call([conv, xdr, back])
        subprocess.check_call([conv, src, direct])
        assert open(back, "rb").read() == open(direct, "rb").read()
        a, b = meshes.read_xda(src), meshes.read_xda(back)
        np.testing.assert_array_equal(a.xyz, b.xyz)
        np.testing.assert_array_equal(a.tri, b.tri)
        np.testing.assert_array_equal(a.quad, b.quad)
        assert a.bcs == b.bcs
        raw = open(xdr, "rb").read()
        n_el, n_no = len(a.tri) + len(a.quad), len(a.xyz)
        head = (b"\x00\x00\x00\x0elibMesh-0.7.0+\x00\x00" + n_el.to_bytes(4, "big") + n_no.to_bytes(4, "big") +
                b"\x00\x00\x00\x01.\x00\x00\x00" + 3 * b"\x00\x00\x00\x03n/a\x00" + n_el.to_bytes(4, "big"))
        assert raw.startswith(head)
        words = 4 * len(a.tri) + 5 * len(a.quad)
        assert len(raw) == len(head) + 4 * words + 24 * n_no + 4 + 12 * len(a.bcs)
        first = np.frombuffer(raw[len(head) + 4 * words:len(head) + 4 * words + 24], dtype=">f8")
        np.testing.assert_array_equal(first, a.xyz[0])
    msh = tmp_path / "two.msh"
    msh.write_text(MSH_EXAMPLE)
    subprocess.check_call([conv, str(msh), str(tmp_path / "two.xdr")])
    subprocess.check_call([conv, str(tmp_path / "two.xdr"), str(tmp_path / "two.xda")])
    txt = open(tmp_path / "two.xda").read()
    assert txt.startswith("libMesh-0.9.2+") and "# number of nodesets" in txt
    subprocess.check_call([conv, str(tmp_path / "two.xda"), str(tmp_path / "two2.xdr")])
    assert open(tmp_path / "two.xdr", "rb").read() == open(tmp_path / "two2.xdr", "rb").read()


def _read_exodus(path):
    from scipy.io import netcdf_file

    with netcdf_file(path, "r", mmap=False) as f:
        out = {"dims": dict(f.dimensions), "title": f.title.decode(), "word": int(f.floating_point_word_size)}
        for k, v in f.variables.items():
            out[k] = np.array(v[:])
            if hasattr(v, "elem_type"):
                out[k + ".elem_type"] = v.elem_type.decode()
    return out


@pytest.mark.parametrize("name", ["test_A_uv_t", "test_B_uv_q"])
def test_exodus_file_reads_back(tools, tmp_path, name):
    """fem-shell.cpp:1240-1251 writes "<out>.e" through libMesh's ExodusII_IO; here the file is a hand-written classic
    netCDF (CDF-2) file with ExodusII's dimensions and variables (host/mesh_io.cpp write_exodus).  Read back with scipy's
    netCDF reader: displaced coordinates, 1-based connectivity per element block, the six nodal variables."""
    conv = os.path.join(HOST, "meshConvert")
    src = os.path.join(meshes.MESH_DIR, name + ".xda")
    out = str(tmp_path / (name + ".e"))
    subprocess.check_call([conv, src, out, "ramp"])
    assert open(out, "rb").read(4) == b"CDF\x02"
    m = meshes.read_xda(src)
    e = _read_exodus(out)
    n = m.n_nodes
    assert e["dims"]["num_nodes"] == n and e["dims"]["num_elem"] == len(m.tri) + len(m.quad) and e["dims"]["num_dim"] == 3
    assert e["dims"]["time_step"] is None and e["dims"]["num_nod_var"] == 6 and e["word"] == 8
    u = 1e-3 * np.outer(np.arange(1, n + 1), np.arange(1, 7))
    for d, c in enumerate("xyz"):
        np.testing.assert_allclose(e["coord" + c], m.xyz[:, d] + u[:, d], rtol=1e-15, atol=1e-17)  # the displaced mesh (fem-shell.cpp:172-175)
    names = ["".join(ch.decode() for ch in row).rstrip("\x00") for row in e["name_nod_var"]]
    assert names == ["u", "v", "w", "tx", "ty", "tz"]
    for v in range(6):
        np.testing.assert_allclose(e["vals_nod_var%d" % (v + 1)], u[None, :, v], rtol=1e-15, atol=0)
    np.testing.assert_array_equal(e["time_whole"], [0.0])
    conn = m.tri if len(m.tri) else m.quad
    assert e["connect1.elem_type"] == ("TRI3" if len(m.tri) else "QUAD4")
    np.testing.assert_array_equal(e["connect1"], conn + 1)
    np.testing.assert_array_equal(e["elem_num_map"], np.arange(1, len(conn) + 1))
    np.testing.assert_array_equal(e["node_num_map"], np.arange(1, n + 1))


def test_gmsh_boundary_lines_are_resolved_through_a_side_table(tools, tmp_path):
    """every boundary line used to scan all elements (quadratic); 160k triangles with 1600 boundary lines
    must read in a blink, and the sides found are those a scan finds (first element in file order)."""
    import time

    n = 282
    m = meshes.structured(n, n, 0, 0, 1, 1, kind="t", ul_lr=True, bcids=(0, 0, 1, 1), factor=1.0, loading=0)
    lines = ["$MeshFormat", "2.2 0 8", "$EndMeshFormat", "$Nodes", str(m.n_nodes)]
    lines += ["%d %.17g %.17g %.17g" % (i + 1, *m.xyz[i]) for i in range(m.n_nodes)]
    el = ["%d 2 2 0 0 %d %d %d" % (e + 1, *(m.tri[e] + 1)) for e in range(len(m.tri))]
    for (e, s, bid) in m.bcs:
        a, b = m.tri[e][s], m.tri[e][(s + 1) % 3]
        el.append("%d 1 2 %d 0 %d %d" % (len(el) + 1, bid, b + 1, a + 1))  # reversed: orientation must not matter
    lines += ["$EndNodes", "$Elements", str(len(el))] + el + ["$EndElements"]
    p = tmp_path / "big.msh"
    p.write_text("\n".join(lines) + "\n")
    conv = os.path.join(HOST, "meshConvert")
    t0 = time.time()
    subprocess.check_call([conv, str(p), str(tmp_path / "big.xda")])
    assert time.time() - t0 < 20.0
    got = meshes.read_xda(str(tmp_path / "big.xda"))
    np.testing.assert_array_equal(got.tri, m.tri)
    assert sorted(got.bcs) == sorted(m.bcs)
    np.testing.assert_array_equal(got.dirichlet_mask(), m.dirichlet_mask())


def test_xda_side_index_is_range_checked(tools, tmp_path):
    fem, _ = tools
    src = open(os.path.join(meshes.MESH_DIR, "test_A_uv_t.xda")).read().rstrip("\n").split("\n")
    src[-1] = "0 3 0"  # side 3 of a triangle
    p = tmp_path / "bad.xda"
    p.write_text("\n".join(src) + "\n")
    r = subprocess.run([fem, "-nu", "0.25", "-e", "30000", "-t", "1", "-mesh", str(p)], capture_output=True, text=True)
    assert r.returncode != 0 and "names side 3 of an element with 3 sides" in r.stderr


def test_petsc_style_options_are_understood(tools):
    fem, _ = tools
    mesh = os.path.join(meshes.MESH_DIR, "test_A_uv_t.xda")
    base = [fem, "-nu", "0.25", "-e", "30000", "-t", "1.0", "-mesh", mesh]
    r = subprocess.run(base + ["-pc_type", "nonsense"], capture_output=True, text=True)
    assert r.returncode != 0 and "-pc_type nonsense is not available" in r.stderr
    for pc in ("ilu", "none"):  # PETSc's serial default and "none": a note saying what runs, like an unavailable -ksp_type
        r = subprocess.run(base + ["-pc_type", pc], capture_output=True, text=True)
        assert "NOTE: -pc_type %s is not available on the GPU; using the 6x6 block-Jacobi" % pc in r.stderr
    r = subprocess.run(base + ["-ksp_type", "gmres", "-pc_type", "bjacobi"], capture_output=True, text=True)
    assert "using -ksp_type cg" in r.stderr


@pytest.mark.gpu
def test_cli_with_the_multigrid_preconditioner(tools):
    fem, _ = tools
    mesh = os.path.join(meshes.MESH_DIR, "test_G_mpi_64_q.xda")
    base = [fem, "-nu", "0.3", "-e", "1e7", "-t", "0.5", "-mesh", mesh]
    a = subprocess.run(base + ["-ksp_type", "cg", "-pc_type", "gamg", "-ksp_rtol", "1e-12"], capture_output=True, text=True)
    assert a.returncode == 0, a.stderr
    assert "multigrid-preconditioned CG" in a.stdout
    ua = parse_solution(a.stdout)
    assert ua[2112, 2] == pytest.approx(0.106465, abs=6e-7)  # doc/validation.tex:518
    b = subprocess.run(base + ["-pc_type", "bjacobi"], capture_output=True, text=True)
    assert b.returncode == 0 and "6x6 block-Jacobi CG" in b.stdout
    ub = parse_solution(b.stdout)
    ita = int(re.search(r"(\d+) iterations", a.stdout).group(1))
    itb = int(re.search(r"(\d+) iterations", b.stdout).group(1))
    assert itb > 10 * ita
    assert np.abs(ua - ub).max() <= 1e-9 * np.abs(ub).max()


@pytest.mark.gpu
def test_cli_defaults_converge_on_a_256_squared_panel(tools, tmp_path):
    """No -pc_type, no -max_it: the stand-alone program picks the multigrid and libMesh's iteration limit of 5000 (the
    reference's own default, PETSc's GMRES + ILU, is also stronger than point-block Jacobi, which needs about 40,000
    iterations on this mesh and does not converge at all on the 4M-triangle ones)."""
    fem, meshgen = tools
    name = str(tmp_path / "panel256")
    subprocess.check_call([meshgen, "t", "256", "256", "0", "0", "10", "10", "0,0,0,0", "300", "2", "1", "z", name])
    r = subprocess.run([fem, "-nu", "0.3", "-e", "1e7", "-t", "0.5", "-mesh", name + ".xda"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "multigrid-preconditioned CG" in r.stdout and "NOT converged" not in r.stdout
    assert int(re.search(r"(\d+) iterations", r.stdout).group(1)) < 300
    u = parse_solution(r.stdout)
    assert u[128 * 257 + 128, 2] == pytest.approx(0.1064, rel=2e-3)  # the plate of Test D / G (doc/validation.tex:289, 518)


def _run_ranks(cmd, world, tmp_path):
    fake = os.path.join(ROOT, "tests", "helpers", "fake_rccl")
    subprocess.check_call(["make", "-C", fake, "-s"])
    procs = []
    for r in range(world):
        env = dict(os.environ, FEMSHELL_RANK=str(r), FEMSHELL_WORLD_SIZE=str(world), FEMSHELL_DEVICE="0",
                   FEMSHELL_UID_FILE=str(tmp_path / ("uid_%d" % world)), FEMSHELL_RCCL_LIB=os.path.join(fake, "libfake_rccl.so"))
        procs.append(subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    return outs


@pytest.mark.gpu
def test_stand_alone_program_on_two_ranks(tools, tmp_path):
    # Test G's mode (mpirun -n 2, run_examples.sh:47-48): two processes, each with its row range, RCCL id through a
    # file; the ranks share the one GPU of the test box through the fake RCCL transport
    fem, _ = tools
    mesh = os.path.join(meshes.MESH_DIR, "test_G_mpi_64_q.xda")
    cmd = [fem, "-nu", "0.3", "-e", "1e7", "-t", "0.5", "-mesh", mesh]
    single = subprocess.run(cmd, capture_output=True, text=True)  # (the program's default: the multigrid preconditioner)
    assert single.returncode == 0, single.stderr
    outs = _run_ranks(cmd, 2, tmp_path)
    assert [rc for rc, _, _ in outs] == [0, 0], outs
    assert "multigrid-preconditioned CG" in single.stdout and "multigrid-preconditioned CG" in outs[0][1]
    assert "(2 ranks)" in outs[0][1] and "Solution:" not in outs[1][1]  # rank 0 reports
    u1, u2 = parse_solution(single.stdout), parse_solution(outs[0][1])
    assert u2[2112, 2] == pytest.approx(0.106465, abs=6e-7)
    assert np.abs(u1 - u2).max() <= 1e-8 * np.abs(u1).max()


@pytest.mark.gpu
def test_coupled_program_on_two_ranks(tools, coupled_tool, tmp_path):
    # BASELINE configs[4] is a 2-GPU coupled run: the coupled program partitions the structure solve over the ranks
    # while the in-process coupling stand-in runs replicated; scaled flap, 2 ranks against 1
    _, meshgen = tools
    name = str(tmp_path / "flap")
    subprocess.check_call([meshgen, "t", "10", "100", "0", "0", "0.1", "1", "2,20,2,2", "1", "0", "1", "y", name])
    cmd = [coupled_tool, "-nu", "0.3", "-e", "1e6", "-t", "0.1", "-mesh", name + ".xda", "-config", CONFIG, "-dt", "0.01",
           "-axis", "y", "-steps", "3", "-fluid", "edge"]
    single = subprocess.run(cmd + ["-pc_type", "bjacobi", "-max_it", "100000"], capture_output=True, text=True)
    assert single.returncode == 0, single.stderr
    outs = _run_ranks(cmd + ["-pc_type", "bjacobi", "-max_it", "100000"], 2, tmp_path)
    assert [rc for rc, _, _ in outs] == [0, 0], outs
    tips1 = [float(v) for v in re.findall(r"tip\[\d+\] node \d+ = (\S+)", single.stdout)]
    tips2 = [float(v) for v in re.findall(r"tip\[\d+\] node \d+ = (\S+)", outs[0][1])]
    assert len(tips1) == 3 and len(tips2) == 3 and "tip[" not in outs[1][1]
    np.testing.assert_allclose(tips2, tips1, rtol=1e-7)
    # the same with the programs' default, the multigrid preconditioner: row-partitioned hierarchy (csrc/amg_dist.cpp), K and
    # the hierarchy once for all coupling iterations, same tip displacements
    outs_mg = _run_ranks(cmd, 2, tmp_path)
    assert [rc for rc, _, _ in outs_mg] == [0, 0], outs_mg
    tips3 = [float(v) for v in re.findall(r"tip\[\d+\] node \d+ = (\S+)", outs_mg[0][1])]
    np.testing.assert_allclose(tips3, tips1, rtol=1e-7)
    its = lambda out: int(re.search(r"(\d+) CG iterations", out).group(1))
    assert its(outs_mg[0][1]) * 3 < its(outs[0][1])


@pytest.mark.gpu
def test_coupled_program_writes_one_output_per_converged_time_step(tools, coupled_tool, tmp_path):
    """fem-shell_precice.cpp:393 calls writeOutput(mesh, es, t) after every converged time step, and :1526-1560 names the
    files: <out>_NNNN.e (ExodusII) when several processes run, <out>_NNN.pvtu (VTK XML, with its piece) in a serial run.
    Same names and the same content here: the displaced mesh of that step and its six nodal variables."""
    import xml.etree.ElementTree as ET

    _, meshgen = tools
    name = str(tmp_path / "flap")
    subprocess.check_call([meshgen, "t", "6", "40", "0", "0", "0.1", "1", "2,20,2,2", "1", "0", "1", "y", name])
    m = meshes.read_xda(name + ".xda")
    cmd = [coupled_tool, "-nu", "0.3", "-e", "1e6", "-t", "0.1", "-mesh", name + ".xda", "-config", CONFIG, "-dt", "0.01",
           "-axis", "y", "-steps", "3", "-fluid", "edge"]
    serial = subprocess.run(cmd + ["-out", str(tmp_path / "ser")], capture_output=True, text=True)
    assert serial.returncode == 0, serial.stderr
    tips = [float(v) for v in re.findall(r"tip\[\d+\] node \d+ = (\S+)", serial.stdout)]
    probe = int(re.search(r"tip\[0\] node (\d+)", serial.stdout).group(1))
    for t in range(3):
        index = tmp_path / ("ser_%03d.pvtu" % t)
        piece = tmp_path / ("ser_%03d_0.vtu" % t)
        assert index.exists() and piece.exists()
        assert ET.parse(index).getroot().find(".//Piece").get("Source") == piece.name
        root = ET.parse(piece).getroot()
        pc = root.find(".//Piece")
        assert int(pc.get("NumberOfPoints")) == m.n_nodes and int(pc.get("NumberOfCells")) == len(m.tri)
        arrays = {a.get("Name"): np.array(a.text.split(), dtype=float) for a in root.iter("DataArray") if a.get("Name")}
        assert arrays["u"][probe] == pytest.approx(tips[t], rel=1e-5)  # the step's own solution (six printed digits), not the last one
        assert t == 0 or abs(arrays["u"][probe] - tips[t - 1]) > 1e-4 * abs(tips[t])
        pts = np.array(root.find(".//Points/DataArray").text.split(), dtype=float).reshape(-1, 3)
        disp = np.stack([arrays["u"], arrays["v"], arrays["w"]], axis=1)
        np.testing.assert_allclose(pts, m.xyz + disp, rtol=0, atol=1e-12)  # displaced nodes (PC:380-390)
        np.testing.assert_array_equal(arrays["connectivity"].reshape(-1, 3).astype(int), m.tri)
        assert set(arrays["types"].astype(int)) == {5} and arrays["offsets"][-1] == 3 * len(m.tri)
    assert not (tmp_path / "ser_003.pvtu").exists()
    outs = _run_ranks(cmd + ["-out", str(tmp_path / "par")], 2, tmp_path)
    assert [rc for rc, _, _ in outs] == [0, 0], outs
    for t in range(3):
        e = _read_exodus(str(tmp_path / ("par_%04d.e" % t)))
        assert e["dims"]["num_nodes"] == m.n_nodes
        assert e["vals_nod_var1"][0][probe] == pytest.approx(tips[t], rel=1e-5)  # (six printed digits)
    assert not (tmp_path / "par_0003.e").exists() and not (tmp_path / "par_000.pvtu").exists()
