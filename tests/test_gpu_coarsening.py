"""Coarsening steps with their numerics on the device (csrc/amg_device_setup.cpp: near_null_row, k_amg_tentative_qr<false|true>,
k_amg_prolongator, k_patch_prolongator, k_amg_ap, k_amg_restriction, k_amg_galerkin / k_amg_galerkin_mfma) held operator by
operator to the restatement oracle/amg_oracle.py, on the meshes and knobs where those kernels can go wrong unseen: curved
normals, masked dofs, coarse rows of more than the 16 blocks one pass of the matrix-core Galerkin kernel covers, aggregates on
both sides of the 42 nodes the register QR holds, K in full storage, the plain rigid-body modes, the default configuration and
the cluster blocks of the patch smoother.  A wrong P or A_c costs iterations, not the answer, so only such comparisons see it
(tests/test_coarsening_reference_cpu.py plants bugs of that kind).  Every case asserts, from the exported or restated hierarchy,
that it reached what it is there for (tests/helpers/hierarchy.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import amg_oracle
from tests.helpers import hierarchy, multirank_worker
from tests.helpers.product import ROOT, ensure_built, pkg
from tests.test_gpu_amg import _fan_mesh, _make, _poor_shell

pytestmark = pytest.mark.gpu


class _Mesh:
    def __init__(self, xyz, tri, quad, dmask, loads, mat):
        self.xyz, self.tri, self.quad, self.dmask, self.loads, self.mat = xyz, tri, quad, dmask, loads, mat


def _mesh(kind, n=None):
    if kind in ("roof", "cylinder", "quads"):
        m, mat = _make(kind, n)
        return _Mesh(m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads, mat)
    if kind == "mixed":  # triangles and quadrilaterals in one mesh (tests/test_gpu_amg.py, patterns test)
        m, mat = _make("quads", n)
        half = len(m.quad) // 2
        tri = np.concatenate([m.quad[half:, [0, 1, 2]], m.quad[half:, [0, 2, 3]]]).astype(np.int32)
        return _Mesh(m.xyz, tri, m.quad[:half], m.dirichlet_mask(), m.loads, mat)
    if kind == "curved_panel":  # z = 0.2 sin(1.1 x) cos(0.6 y), clamped on one side, simply supported on another
        m, mat = multirank_worker.build_problem("panel")
        return _Mesh(m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads, mat)
    if kind == "delaunay":  # jittered grid on a curved shell, shuffled numbering: irregular valence, no slivers
        from tests.test_gpu_parity import delaunay_shell

        xyz, tri = delaunay_shell(n, 4, jittered=True)
        dmask = np.zeros(len(xyz), dtype=np.uint8)
        dmask[xyz[:, 0] < 0.15] = 0x3F
        loads = np.zeros((len(xyz), 6))
        loads[:, 2] = 1.0
        return _Mesh(xyz, tri, None, dmask, loads, (0.3, 7.0e4, 0.03))
    if kind == "fan":  # dished disc of 12 rings of valence n around a hub numbered last, clamped at the rim
        xyz, tri = _fan_mesh(n, 12)
        dmask = np.zeros(len(xyz), dtype=np.uint8)
        dmask[np.hypot(xyz[:, 0], xyz[:, 1]) > 11.5] = 0x3F
        loads = np.zeros((len(xyz), 6))
        loads[:, 2] = 1.0
        return _Mesh(xyz, tri, None, dmask, loads, (0.3, 1e7, 0.2))
    if kind == "poor_shell":  # random Delaunay shell of poor element quality: clusters of rigidly coupled nodes
        xyz, tri, dmask, loads = _poor_shell(n, 2 if n == 3000 else 3, along_x=(n == 20000))
        return _Mesh(xyz, tri, None, dmask, loads, (0.3, 7.0e4, 0.03))
    raise ValueError(kind)


def _solved(m, coarsest_nodes=None, max_it=2000):
    ensure_built()
    fs = pkg.FemShell(*m.mat, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dmask)
    fs.set_loads(m.loads)
    if coarsest_nodes is None:
        fs.set_preconditioner("amg")
    else:
        fs.set_preconditioner("amg", coarsest_nodes=coarsest_nodes)
    _, info = fs.solve(rtol=1e-10, max_it=max_it)
    assert info["converged"] == 1, info
    return fs


def _compare(m, coarsest_nodes=1400, **tol):
    fs = _solved(m, None if coarsest_nodes == 1400 else coarsest_nodes)
    try:
        _, got = hierarchy.compare(fs, m.xyz, m.dmask, m.tri, m.quad, coarsest_nodes=coarsest_nodes, **tol)
    finally:
        fs.close()
    return got


def _curved(m):
    """the node normals of the mesh are not all parallel: every z term of near_null_row and of the projection is in play"""
    nrm = amg_oracle.node_normals(m.xyz, m.tri, m.quad)
    return np.abs(nrm @ nrm[0]).min() < 0.99


def _wide_device_rows(got):
    """steps on the device whose coarse operator has a stored row of more than 16 blocks (a second pass of the matrix cores)"""
    return [li for li, (dev, w) in enumerate(zip(got["device"], got["stored_width"])) if dev and w > hierarchy.GALERKIN_PASS]


# ---- curved meshes with masked dofs: both Galerkin kernels, both storages of the coarse operators


@pytest.mark.parametrize("coarse_sym", ["1", "100000"])
@pytest.mark.parametrize("galerkin", ["valu", "mfma"])
@pytest.mark.parametrize("kind", ["roof", "cylinder"])
def test_curved_meshes_coarsened_on_the_device_follow_the_restatement(monkeypatch, kind, galerkin, coarse_sym):
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    monkeypatch.setenv("FEMSHELL_AMG_GALERKIN", galerkin)
    monkeypatch.setenv("FEMSHELL_AMG_COARSE_SYM", coarse_sym)
    m = _mesh(kind, 48)
    assert _curved(m)
    fs = _solved(m, 60)
    try:
        levels, got = hierarchy.compare(fs, m.xyz, m.dmask, m.tri, m.quad, coarsest_nodes=60)
    finally:
        fs.close()
    assert got["device"][:2] == [True, True], got["device"]
    if galerkin == "mfma":
        # the library's own record of the rows it stored: the matrix-core work follows their widths (compare() holds it to the
        # storage asked for), and it would differ with the other storage
        monkeypatch.setenv("FEMSHELL_AMG_COARSE_SYM", "100000" if coarse_sym == "1" else "1")
        assert got["mfma_flops_issued"] != hierarchy.mfma_flops_issued(levels[0].P, levels[1].A)


def test_second_pass_of_the_matrix_core_galerkin_kernel(monkeypatch):
    """Pinched cylinder 80 x 80: a device-built coarse operator with a row of more than 16 blocks."""
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    monkeypatch.setenv("FEMSHELL_AMG_GALERKIN", "mfma")
    got = _compare(_mesh("cylinder", 80), coarsest_nodes=60)
    assert _wide_device_rows(got), got["stored_width"]


@pytest.mark.parametrize("kind", ["quads", "mixed"])
def test_quadrilaterals_coarsened_on_the_device_follow_the_restatement(monkeypatch, kind):
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    m = _mesh(kind, 40)
    assert m.quad is not None and len(m.quad) and (kind == "quads") == (m.tri is None or len(m.tri) == 0)
    got = _compare(m, coarsest_nodes=60)
    assert got["device"][:2] == [True, True], got["device"]


def test_curved_panel_with_k_in_full_storage(monkeypatch):
    """FEMSHELL_SYMMETRIC=0: K and every coarse operator stored in full (the branches of for_each_neighbour without diag_upper), even
    with FEMSHELL_AMG_COARSE_SYM=1.  The matrix-core Galerkin kernel's work shows the storage the library chose: full rows, not the
    diagonal and upper blocks."""
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", "0")
    monkeypatch.setenv("FEMSHELL_AMG_COARSE_SYM", "1")
    monkeypatch.setenv("FEMSHELL_AMG_GALERKIN", "mfma")
    m = _mesh("curved_panel")
    assert _curved(m)
    fs = _solved(m, 60)
    try:
        levels, got = hierarchy.compare(fs, m.xyz, m.dmask, m.tri, m.quad, coarsest_nodes=60)
    finally:
        fs.close()
    assert got["device"][:2] == [True, True], got["device"]
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", "1")  # (what the issued work would be with the upper blocks stored)
    assert got["mfma_flops_issued"] != hierarchy.mfma_flops_issued(levels[0].P, levels[1].A)


def _plain_rbm_child():
    """(run in a process of its own: the library reads FEMSHELL_AMG_PLAIN_RBM once per process)"""
    assert os.environ.get("FEMSHELL_AMG_PLAIN_RBM") == "1"
    m = _mesh("curved_panel")
    assert _curved(m)
    got = _compare(m, coarsest_nodes=60)  # (the restatement without normals: no projection onto the tangent planes)
    assert got["device"][:2] == [True, True], got["device"]


def test_curved_panel_with_the_plain_rigid_body_modes():
    env = dict(os.environ, FEMSHELL_AMG_PLAIN_RBM="1", FEMSHELL_AMG_DEVICE_MIN="100")
    script = "import sys; sys.path.insert(0, %r); from tests.test_gpu_coarsening import _plain_rbm_child; _plain_rbm_child()" % ROOT
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    print(r.stdout.strip())


@pytest.mark.parametrize("galerkin", ["valu", "mfma"])
def test_jittered_delaunay_shell_in_generator_numbering(monkeypatch, galerkin):
    """5,929 nodes in shuffled numbering, irregular valence, no slivers; levels 5929 / 705 / 45 with coarsest_nodes=60, both steps on
    the device, coarse rows of 18 and 19 blocks.  (Zero blocks stay in the patterns -- the rows of P at clamped nodes --: the restatement
    keeps them as the library does, else its level 2 has 62 nodes.)"""
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    monkeypatch.setenv("FEMSHELL_AMG_GALERKIN", galerkin)
    m = _mesh("delaunay", 6000)
    assert _curved(m)
    got = _compare(m, coarsest_nodes=60)
    assert got["device"] == [True, True], got["device"]
    assert _wide_device_rows(got) == [0, 1], got["stored_width"]


@pytest.mark.parametrize("galerkin", ["valu", "mfma"])
def test_register_and_memory_qr_in_one_step(monkeypatch, galerkin):
    """The fan of valence 80 with 12 rings, coarsest_nodes=20, FEMSHELL_AMG_QR unset: one device step has aggregates of more than
    42 nodes (k_amg_tentative_qr<true>) beside smaller ones (<false>), and a device-built coarse row of more than 16 blocks."""
    monkeypatch.delenv("FEMSHELL_AMG_QR", raising=False)
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    monkeypatch.setenv("FEMSHELL_AMG_GALERKIN", galerkin)
    got = _compare(_mesh("fan", 80), coarsest_nodes=20)
    both = [li for li, (dev, a) in enumerate(zip(got["device"], got["aggregate_nodes"]))
            if dev and a.max() > hierarchy.QR_REGISTER_NODES and a.min() <= hierarchy.QR_REGISTER_NODES]
    assert both, [(dev, a.min(), a.max()) for dev, a in zip(got["device"], got["aggregate_nodes"])]
    assert _wide_device_rows(got), got["stored_width"]


def test_every_aggregate_through_the_memory_qr_on_the_cylinder(monkeypatch):
    monkeypatch.setenv("FEMSHELL_AMG_QR", "memory")
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    got = _compare(_mesh("cylinder", 48), coarsest_nodes=60)
    assert got["device"][:2] == [True, True], got["device"]


@pytest.mark.parametrize("kind,n", [("cylinder", 80), ("roof", 90)])
def test_default_configuration_follows_the_restatement(monkeypatch, kind, n):
    """No knob set: level 0 is coarsened on the device, as in the benchmark, the levels below on the host."""
    for knob in ("FEMSHELL_AMG_DEVICE_MIN", "FEMSHELL_AMG_GALERKIN", "FEMSHELL_AMG_COARSE_SYM", "FEMSHELL_AMG_QR", "FEMSHELL_AMG_SETUP"):
        monkeypatch.delenv(knob, raising=False)
    m = _mesh(kind, n)
    assert len(m.xyz) > 5000
    got = _compare(m)
    assert got["device"][0], got["device"]


# ---- the cluster blocks of the patch smoother (k_patch_prolongator)

# (the inverses of cluster blocks whose nodes nearly coincide -- condition numbers of 1e8 and beyond -- come out of two different
#  factorisations: P of level 0 agrees to the digits those leave, where it agrees to 1e-11 on meshes without clusters; the coarse
#  operators and the prolongators below inherit them and are held to 1e-5, as level 1 is in tests/test_gpu_amg.py)
PATCH_TOL = dict(p_tol=[2e-6, 1e-5], a_tol=[hierarchy.A_TOL, 1e-5])


def test_patch_prolongator_on_the_poor_shell(monkeypatch):
    """The 3,000-point shell of poor element quality, coarsest_nodes=60.  Level 0 has clusters, so its step runs on the device
    whatever FEMSHELL_AMG_DEVICE_MIN says (the host path has no cluster blocks): between the two contexts below its P is
    k_patch_prolongator against itself, the same bits.  The 182-node level below is coarsened on the host by default and on the
    device with FEMSHELL_AMG_DEVICE_MIN=100: that step is device numerics against host numerics, to 1e-11 / 1e-10.  Both contexts
    follow the restatement with the library's labels on every level, the two steps below the glued one included."""
    m = _mesh("poor_shell", 3000)
    out = []
    for dmin in (None, "100"):
        if dmin is not None:
            monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", dmin)
        fs = _solved(m, coarsest_nodes=60)
        try:
            _, got = hierarchy.compare(fs, m.xyz, m.dmask, m.tri, coarsest_nodes=60, **PATCH_TOL)
            sizes = got["sizes"]
            ex = [fs.amg_export(li) for li in range(len(sizes))]
            P = [hierarchy.bsr(e["P_rowptr"], e["P_cols"], e["P_vals"], sizes[li + 1]) for li, e in enumerate(ex[:-1])]
            A = [hierarchy.bsr(e["A_rowptr"], e["A_cols"], e["A_vals"], sizes[li]) for li, e in enumerate(ex)]
        finally:
            fs.close()
        assert got["clusters"] > 500 and len(sizes) >= 3, (got["clusters"], sizes)
        out.append((sizes, got["device"], P, A))
    host, dev = out
    assert host[0] == dev[0], (host[0], dev[0])
    assert host[1][:2] == [True, False] and dev[1][:2] == [True, True], (host[1], dev[1])
    np.testing.assert_array_equal(host[2][0].data, dev[2][0].data)  # (level 0: the same kernel both times)
    for li, (a, b) in enumerate(zip(host[2], dev[2])):
        assert abs(b - a).max() <= hierarchy.P_TOL * abs(a).max(), ("P", li)
    for li, (a, b) in enumerate(zip(host[3], dev[3])):
        assert abs(b - a).max() <= hierarchy.A_TOL * abs(a).max(), ("A", li)


def test_patch_prolongator_on_the_20k_point_shell():
    """The 20,000-point shell numbered along x (device step of level 0 by default) against the restatement with the library's labels.
    More nearly coincident nodes than on the 3,000-point shell: level-0 P agrees to 4e-5 (held to 1e-4), the coarse operator to 2e-9.
    The bound still stands far below what leaving out the cluster blocks' share of the smoothing (k_patch_prolongator) does here."""
    m = _mesh("poor_shell", 20000)
    fs = _solved(m)
    try:
        levels, got = hierarchy.compare(fs, m.xyz, m.dmask, m.tri, p_tol=[1e-4, 1e-5], a_tol=PATCH_TOL["a_tol"])
    finally:
        fs.close()
    assert got["clusters"] > 2000 and got["device"][0], (got["clusters"], got["device"])
    L = levels[0]
    point = amg_oracle.bd_matrix(amg_oracle.block_diag_inverse(L.A))
    _, P_without, _, _ = amg_oracle.coarsen(L.A, L.B, L.lam, patch=(L.patch_label, point))
    assert abs(P_without - L.P).max() >= 100.0 * 1e-4 * abs(L.P).max()
