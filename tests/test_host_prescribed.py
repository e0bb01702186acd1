"""Prescribed displacements and support reactions in the host programs: the -prescribed file reader and the refused flag
combinations (CPU: refused before the program needs a GPU), FEM-shell -prescribed -reactions against the binding (GPU)."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers.product import ROOT, ensure_built

HOST = os.path.join(ROOT, "fem-shell_amd", "host")
NX, NY = 8, 3
NU, E, T = 0.3, 2.0e5, 0.05
W_TIP = 0.02


@pytest.fixture(scope="module")
def tools():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fem-shell_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", HOST, "-s"])
    return os.path.join(HOST, "FEM-shell"), os.path.join(HOST, "FEM-shell-precice")


def cantilever():
    """curved strip of 2 * NX * NY triangles: the edge x = 0 clamped (boundary id 1), u, v, w fixed on the edge x = 4 (id 20)"""
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
    text = "# node  u v w  tx ty tz\n\n"
    for n in tip:
        text += "%d 0 0 %r 9 9 9   # the rotations are free there: ignored\n" % (n, W_TIP)
    pres.write_text(text)
    return str(msh), str(pres)


def test_prescribed_file_parser_and_refused_combinations(tools, tmp_path):
    """a good file is accepted up to the point where the program needs a GPU; a missing file, a short line, a node the mesh does
    not have and the flag combinations are refused before, by exit status and message"""
    fem, coupled = tools
    msh, pres = write_cantilever(tmp_path)
    base = [fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh]
    r = subprocess.run(base + ["-prescribed", pres], capture_output=True, text=True)
    assert "expected 'node u v w tx ty tz'" not in r.stderr and "out of range" not in r.stderr and "n_elem()=48" in r.stdout
    r = subprocess.run(base + ["-prescribed", str(tmp_path / "none")], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open" in r.stderr and "FAILED" in r.stdout
    bad = tmp_path / "bad.prescribed"
    bad.write_text("# a good line, then one without tz\n8 0 0 0.02 0 0 0\n\n17 0 0 0.02 0 0\n")
    r = subprocess.run(base + ["-prescribed", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.prescribed: line 4" in r.stderr and "expected 'node u v w tx ty tz'" in r.stderr
    assert "n_elem()" not in r.stdout  # refused while the command line is read
    bad.write_text("8 0 0 0.02 0 0 0\neight 0 0 0.02 0 0 0\n")
    r = subprocess.run(base + ["-prescribed", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr
    bad.write_text("8 0 0 0.02 0 0 0\n8 0 0 0.03 0 0 0\n")
    r = subprocess.run(base + ["-prescribed", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "listed twice" in r.stderr
    bad.write_text("8 0 0 0.02 0 0 0\n-1 0 0 0.03 0 0 0\n")
    r = subprocess.run(base + ["-prescribed", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "line 2" in r.stderr and "out of range" in r.stderr
    bad.write_text("8 0 0 0.02 0 0 0\n\n%d 0 0 0.03 0 0 0\n" % ((NX + 1) * (NY + 1)))
    r = subprocess.run(base + ["-prescribed", str(bad)], capture_output=True, text=True)
    assert r.returncode != 0 and "bad.prescribed: line 3" in r.stderr and "out of range" in r.stderr and "36 nodes" in r.stderr
    # flag combinations
    for extra in (["-rho", "1e-9", "-modes", "3"], ["-rho", "1e-9", "-dt", "1e-3", "-steps", "2"]):
        r = subprocess.run(base + ["-prescribed", pres] + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "-prescribed does not go together" in r.stderr and "FAILED" in r.stdout
        r = subprocess.run(base + ["-reactions"] + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "-reactions" in r.stderr and "FAILED" in r.stdout
    # the coupled program has neither
    config = str(tmp_path / "no-config.xml")
    for extra in (["-prescribed", pres], ["-reactions"]):
        r = subprocess.run([coupled, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-config", config, "-dt", "0.01"] + extra,
                           capture_output=True, text=True)
        assert r.returncode != 0 and extra[0] in r.stderr and "FAILED" in r.stdout


@pytest.mark.gpu
def test_twin_with_prescribed_values_and_reactions_equals_the_binding(tools, tmp_path):
    from tests.test_host_tools import _read_exodus

    pkg = ensure_built()
    fem, _ = tools
    msh, pres = write_cantilever(tmp_path)
    xyz, tri, clamped, tip, loads = cantilever()
    n = len(xyz)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri)
    mask = np.zeros(n, np.uint8)
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
    r = fs.reactions()
    out = str(tmp_path / "P")
    run = subprocess.run([fem, "-nu", repr(NU), "-e", repr(E), "-t", repr(T), "-mesh", msh, "-prescribed", pres, "-reactions", "-out", out],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    ex = _read_exodus(out + ".e")
    got = np.stack([ex["vals_nod_var%d" % (v + 1)][0] for v in range(6)], axis=1)
    assert np.linalg.norm(got - u) <= 1e-12 * np.linalg.norm(u)
    rows = [l.split() for l in open(out + "_reactions.txt").read().splitlines()]
    assert rows[-1][0] == "sum" and [int(q[0]) for q in rows[:-1]] == sorted(np.flatnonzero(mask).tolist())
    listed = np.array([[float(v) for v in q[1:]] for q in rows[:-1]])
    assert np.linalg.norm(listed - r[mask != 0]) <= 1e-12 * np.linalg.norm(r[mask != 0])
    total = np.array([float(v) for v in rows[-1][1:]])
    assert np.abs(total - r.sum(axis=0)).max() <= 1e-12 * np.abs(r).max() * n
    # the sum line balances the loads: the translations are in the null space of K_unc, so the force columns of K_unc u vanish
    # in the sum whatever u is -- to the rounding of the products, 1e-12 of the rows' scales as in tests/test_gpu_prescribed.py
    from tests.helpers import oracle, prescribed as pr

    K_unc, _ = pr.matrices(xyz, tri, None, oracle.material(NU, E, T), mask)
    assert np.abs(total[:3] + loads[:, :3].sum(axis=0)).max() <= 1e-12 * pr.row_scale(K_unc, u).sum()
    # the point arrays of the VTK file
    lines = open(out + ".vtk").read().splitlines()
    for name, cols in (("reaction_f", slice(0, 3)), ("reaction_m", slice(3, 6))):
        at = lines.index("VECTORS %s double" % name)
        arr = np.array([[float(v) for v in l.split()] for l in lines[at + 1:at + 1 + n]])
        assert np.linalg.norm(arr - r[:, cols]) <= 1e-12 * np.linalg.norm(r[:, cols])
    fs.close()
