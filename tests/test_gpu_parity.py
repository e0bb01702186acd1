"""GPU parity tests proper: the HIP path, called through the C ABI, against the CPU oracle on
the same inputs.  Tolerances (FP64): element matrices and assembled K <= 1e-12 relative
(Frobenius / max-entry scaled); displacements < 1e-10 relative to the oracle's direct solve
where CG can attain it (small meshes), otherwise as stated per test."""
import os

import numpy as np
import pytest

from tests.helpers import meshes, oracle, truth
from tests.helpers.product import ensure_built

pytestmark = pytest.mark.gpu
pkg = ensure_built()


def make_ctx(m, nu, E, t, flags=None, with_bc=True, with_loads=True):
    fs = pkg.FemShell(nu, E, t, flags=pkg.REF_DEFAULT if flags is None else flags)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    if with_bc:
        fs.set_dirichlet(m.dirichlet_mask())
    if with_loads:
        fs.set_loads(m.loads)
    return fs


def random_tris(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.normal(size=(3 * n, 3)) * rng.uniform(0.1, 10.0, size=(3 * n, 1))
    tri = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return xyz, tri


# ------------------------------------------------------------------ element matrices

@pytest.mark.parametrize("flags", [3, 2, 1, 0])
def test_element_matrices_random_3d_triangles(flags):
    xyz, tri = random_tris(257, seed=11 + flags)
    fs = pkg.FemShell(0.3, 2.1e5, 0.37, flags=flags)
    fs.set_mesh(xyz, tri)
    Ke = fs.element_matrices(0, len(tri))
    mat = oracle.material(0.3, 2.1e5, 0.37, flags)
    worst = 0.0
    for e in range(len(tri)):
        ref = oracle.element_tri3(xyz[tri[e]], mat)
        worst = max(worst, np.linalg.norm(Ke[e] - ref) / np.linalg.norm(ref))
    assert worst <= 1e-12, worst


def test_element_matrices_special_shapes():
    # axis-aligned isosceles, 2:1 right, obtuse skew in 3-D, near-degenerate sliver
    shapes = [
        [[0, 0, 0], [1, 0, 0], [0, 1, 0]],
        [[0, 0, 0], [2, 0, 0], [0, 1, 0]],
        [[0.3, -1.0, 2.0], [4.1, 0.2, 2.5], [-2.0, 0.7, 3.1]],
        [[0, 0, 0], [1, 0, 0], [0.5, 1e-3, 0]],
        [[5, 5, 5], [5, 6, 5], [5, 5, 6.5]],
    ]
    xyz = np.array(shapes, dtype=np.float64).reshape(-1, 3)
    tri = np.arange(len(xyz), dtype=np.int32).reshape(-1, 3)
    fs = pkg.FemShell(0.25, 30000.0, 1.0)
    fs.set_mesh(xyz, tri)
    Ke = fs.element_matrices(0, len(tri))
    mat = oracle.material(0.25, 30000.0, 1.0)
    for e in range(len(tri)):
        ref = oracle.element_tri3(xyz[tri[e]], mat)
        assert np.linalg.norm(Ke[e] - ref) <= 1e-11 * np.linalg.norm(ref), e
        assert np.abs(Ke[e] - Ke[e].T).max() <= 1e-12 * np.abs(Ke[e]).max()


def test_element_matrices_match_committed_goldens():
    g = np.load(meshes.GOLDEN + "/tri3_elements.npz")
    fs = pkg.FemShell(float(g["nu"]), float(g["E"]), float(g["t"]))
    fs.set_mesh(g["xyz"], g["tri"])
    Ke = fs.element_matrices(0, len(g["tri"]))
    for e in range(len(g["tri"])):
        assert np.linalg.norm(Ke[e] - g["Ke"][e]) <= 1e-12 * np.linalg.norm(g["Ke"][e])


def test_quad4_element_matrices_match_committed_goldens():
    g = np.load(meshes.GOLDEN + "/quad4_elements.npz")
    fs = pkg.FemShell(float(g["nu"]), float(g["E"]), float(g["t"]))
    fs.set_mesh(g["xyz"], None, g["quad"])
    Ke = fs.element_matrices(0, len(g["quad"]))
    for e in range(len(g["quad"])):
        assert np.linalg.norm(Ke[e] - g["Ke"][e]) <= 1e-12 * np.linalg.norm(g["Ke"][e])


@pytest.mark.parametrize("name", ["test_A_uv_t", "test_B_uv_q", "test_C_w_tA16", "test_D_w_q_uni16", "test_E_uvw_t",
                                  "test_F_032_ss_uni", "test_G_mpi_64_q"])
def test_example_solutions_match_committed_goldens(name):
    """whole displacement vectors of the reference's shipped examples against tests/golden/example_solutions.npz
    (refined direct solves of the oracle system) through the multigrid-preconditioned solve with its refinement pass:
    one bound for all seven.  The solver term is 1e-15 ... 1e-13 (tests/test_gpu_amg.py holds it against the direct solve
    of the GPU's own matrix); what remains is the sensitivity of the solution to the 1e-16 rounding differences of two
    FP64 assemblies, largest on the thin plate F and the 64x64 mesh G (1.4e-10).  Block-Jacobi CG alone needed
    tolerances of 1e-6 (F) and 1e-7 (G) here."""
    sols = np.load(meshes.GOLDEN + "/example_solutions.npz")
    nu, E, t = sols[name + "_params"]
    m = meshes.load_example(name)
    fs = make_ctx(m, nu, E, t)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=2000)
    assert info["converged"] == 1 and info["refine_passes_done"] >= 1
    err = np.linalg.norm(u - sols[name]) / np.linalg.norm(sols[name])
    assert err < 2e-10, err
    assert 0.0 <= info["error_estimate"] < 1e-10, info


def random_quads(n, seed):
    """planar, convex, randomly placed and oriented quadrilaterals"""
    rng = np.random.default_rng(seed)
    xyz = np.zeros((4 * n, 3))
    for e in range(n):
        base = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float64)
        base += rng.uniform(-0.25, 0.25, size=(4, 2))
        base *= rng.uniform(0.2, 5.0)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        xyz[4 * e:4 * e + 4] = (np.c_[base, np.zeros(4)] @ q.T) + rng.normal(size=3) * 3.0
    quad = np.arange(4 * n, dtype=np.int32).reshape(n, 4)
    return xyz, quad


@pytest.mark.parametrize("flags", [3, 0])
def test_element_matrices_random_planar_quads(flags):
    xyz, quad = random_quads(129, seed=5 + flags)
    fs = pkg.FemShell(0.3, 2.1e5, 0.37, flags=flags)
    fs.set_mesh(xyz, None, quad)
    Ke = fs.element_matrices(0, len(quad))
    assert Ke.shape == (len(quad), 24, 24)
    mat = oracle.material(0.3, 2.1e5, 0.37, flags)
    worst = 0.0
    for e in range(len(quad)):
        ref = oracle.element_quad4(xyz[quad[e]], mat)
        worst = max(worst, np.linalg.norm(Ke[e] - ref) / np.linalg.norm(ref))
    assert worst <= 1e-12, worst


def test_mixed_tri_quad_mesh_matches_oracle():
    # left half quads, right half triangles, curved so that every element has its own frame...
    # quads must stay planar: bend only along x (cylindrical surface), rows of constant x are straight
    q = meshes.structured(6, 9, 0, 0, 3, 4.5, kind="q", bcids=(-1, 1, -1, -1))
    t = meshes.structured(6, 9, 3, 0, 6, 4.5, kind="t", ul_lr=True)
    # merge: the triangle mesh's left column coincides with the quad mesh's right column
    nq = q.n_nodes
    remap = np.arange(t.n_nodes) + nq
    for j in range(10):
        remap[j * 7] = j * 7 + 6
    keep = np.ones(t.n_nodes, dtype=bool)
    keep[::7] = False
    new_id = np.cumsum(keep) - 1 + nq
    final = np.where(keep, new_id, remap)
    xyz = np.vstack([q.xyz, t.xyz[keep]])
    tri = final[t.tri].astype(np.int32)
    xyz[:, 2] = 0.4 * np.sin(0.9 * xyz[:, 0])  # z depends on x only; quad edges along y stay parallel
    dmask = np.zeros(len(xyz), dtype=np.uint8)
    dmask[:7] = 0x3F
    rng = np.random.default_rng(2)
    loads = rng.normal(size=(len(xyz), 6))
    fs = pkg.FemShell(0.3, 5.0e4, 0.08)
    fs.set_mesh(xyz, tri, q.quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.assemble()
    _, _, vals, F = fs.export_bsr()
    mat = oracle.material(0.3, 5.0e4, 0.08)
    r0, c0, v0, F0 = oracle.assemble(xyz, tri, q.quad, mat, dmask, loads)
    assert np.abs(vals - v0).max() <= 1e-12 * np.abs(v0).max()
    u, info = fs.solve(rtol=1e-13, max_it=100000)
    u0 = oracle.direct_solve(r0, c0, v0, F0)
    assert info["converged"] == 1
    assert np.linalg.norm(u.ravel() - u0) <= 1e-9 * np.linalg.norm(u0)


# ------------------------------------------------------------------ assembled K, F, SpMV

@pytest.mark.parametrize("name,nu,E,t", [("test_A_uv_t", 0.25, 30000.0, 1.0), ("test_C_w_tA16", 0.3, 10.92, 1.0),
                                         ("test_E_uvw_t", 0.25, 10000.0, 0.25),
                                         ("bending_tower_tri_test", 0.3, 1e6, 0.1),
                                         ("test_B_uv_q", 0.25, 30000.0, 1.0), ("test_D_w_q_uni16", 0.3, 1e7, 0.5),
                                         ("test_F_032_ss_uni", 0.3, 1.7472e7, 0.01)])
def test_assembled_matrix_equals_oracle(name, nu, E, t):
    m = meshes.load_example(name)
    fs = make_ctx(m, nu, E, t)
    fs.assemble()
    rowptr, colidx, vals, F = fs.export_bsr()
    mat = oracle.material(nu, E, t)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), m.loads)
    np.testing.assert_array_equal(rowptr, r0)
    np.testing.assert_array_equal(colidx, c0)
    assert np.linalg.norm(vals - v0) <= 1e-12 * np.linalg.norm(v0)
    assert np.abs(vals - v0).max() <= 1e-12 * np.abs(v0).max()
    np.testing.assert_array_equal(F, F0)
    if name in FLAT_EXAMPLES:
        # a flat mesh in the xy plane: membrane (u, v), bending (w, rx, ry) and drilling (rz) entries are disjoint, and on a
        # thin plate (F: t/h = 1e-3 .. 1e-2) the bending entries are far below the membrane entries that set the scale of
        # the bounds above.  Each class on the scale of its own largest entry.
        assert np.ptp(m.xyz[:, 2]) == 0.0
        for cls, mask in truth.class_masks(1, 2).items():
            if cls != "cross":
                assert np.abs(vals - v0)[:, mask].max() <= 1e-12 * np.abs(v0[:, mask]).max(), cls


FLAT_EXAMPLES = ("test_A_uv_t", "test_B_uv_q", "test_C_w_tA16", "test_D_w_q_uni16", "test_F_032_ss_uni")


def curved_mesh(nx, ny, seed=3):
    m = meshes.structured(nx, ny, 0, 0, 4, 3, kind="t", ul_lr=bool(seed & 1), bcids=(0, -1, 1, -1))
    rng = np.random.default_rng(seed)
    m.xyz[:, 2] = 0.3 * np.sin(1.3 * m.xyz[:, 0]) * np.cos(0.7 * m.xyz[:, 1])
    m.xyz[:, :2] += rng.uniform(-0.02, 0.02, size=(m.n_nodes, 2))
    m.loads = rng.normal(size=(m.n_nodes, 6))
    return m


def test_assembly_spmv_on_curved_ragged_mesh():
    m = curved_mesh(37, 29)  # 1140 nodes: last slice is ragged (1140 = 35*32 + 20)
    fs = make_ctx(m, 0.3, 7.0e4, 0.05)
    fs.assemble()
    mat = oracle.material(0.3, 7.0e4, 0.05)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), m.loads)
    _, _, vals, F = fs.export_bsr()
    assert np.abs(vals - v0).max() <= 1e-12 * np.abs(v0).max()
    np.testing.assert_array_equal(F, F0)
    rng = np.random.default_rng(5)
    x = rng.normal(size=6 * m.n_nodes)
    y = fs.spmv(x)
    y0 = oracle.spmv(r0, c0, v0, x)
    assert np.linalg.norm(y - y0) <= 1e-13 * np.linalg.norm(y0)


def test_assembly_is_bitwise_reproducible():
    m = curved_mesh(20, 20)
    fs = make_ctx(m, 0.3, 7.0e4, 0.05)
    fs.assemble()
    a = fs.export_bsr()[2].copy()
    fs.assemble()
    b = fs.export_bsr()[2]
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ solve

def test_known_answers_on_device():
    # thesis values (doc/validation.tex:62-65, 200) straight from the HIP path
    m = meshes.load_example("test_A_uv_t")
    fs = make_ctx(m, 0.25, 30000.0, 1.0)
    u, info = fs.solve(rtol=1e-12, max_it=5000)
    assert info["converged"] == 1
    assert u[22, 0] == pytest.approx(-0.0255988, abs=6e-8)
    assert u[26, 1] == pytest.approx(0.1944070, abs=6e-7)
    m = meshes.load_example("test_C_w_tA16")
    fs = make_ctx(m, 0.3, 10.92, 1.0)
    u, info = fs.solve(rtol=1e-12, max_it=20000)
    assert info["converged"] == 1
    assert u[144, 2] == pytest.approx(1.15169, abs=6e-6)
    # quads: B (:133-136), D (:289), F (:474), G (:518)
    m = meshes.load_example("test_B_uv_q")
    u, info = make_ctx(m, 0.25, 30000.0, 1.0).solve(rtol=1e-12, max_it=20000)
    assert info["converged"] == 1
    assert u[22, 0] == pytest.approx(-0.0427728, abs=6e-8) and u[26, 1] == pytest.approx(0.3160560, abs=6e-7)
    m = meshes.load_example("test_D_w_q_uni16")
    u, info = make_ctx(m, 0.3, 1e7, 0.5).solve(rtol=1e-12, max_it=50000)
    assert info["converged"] == 1 and u[144, 2] == pytest.approx(0.106454, abs=6e-7)
    m = meshes.load_example("test_F_032_ss_uni")
    u, info = make_ctx(m, 0.3, 1.7472e7, 0.01).solve(rtol=1e-12, max_it=200000)
    assert info["converged"] == 1 and u[544, 2] == pytest.approx(12.9640e-6, abs=6e-11)
    m = meshes.load_example("test_G_mpi_64_q")
    u, info = make_ctx(m, 0.3, 1e7, 0.5).solve(rtol=1e-12, max_it=200000)
    assert info["converged"] == 1 and u[2112, 2] == pytest.approx(0.106465, abs=6e-7)


@pytest.mark.parametrize("name,nu,E,t", [("test_A_uv_t", 0.25, 30000.0, 1.0), ("test_C_w_tA16", 0.3, 10.92, 1.0),
                                         ("test_E_uvw_t", 0.25, 10000.0, 0.25)])
def test_displacements_match_oracle_direct_solve(name, nu, E, t):
    m = meshes.load_example(name)
    fs = make_ctx(m, nu, E, t)
    u, info = fs.solve(rtol=1e-13, max_it=50000)
    mat = oracle.material(nu, E, t)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), m.loads)
    u0 = oracle.direct_solve(r0, c0, v0, F0)
    err = np.linalg.norm(u.ravel() - u0) / np.linalg.norm(u0)
    assert info["converged"] == 1
    assert err < 1e-10, err
    # true residual of the returned solution
    res = np.linalg.norm(F0 - oracle.spmv(r0, c0, v0, u.ravel())) / np.linalg.norm(F0)
    assert res < 1e-11, res


def test_cg_follows_oracle_cg_iteration_by_iteration():
    m = meshes.structured(16, 16, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    fs = make_ctx(m, 0.3, 1e7, 0.5)
    u, info = fs.solve(rtol=1e-10, max_it=5000)
    mat = oracle.material(0.3, 1e7, 0.5)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), m.loads)
    u0, info0 = oracle.pcg(r0, c0, v0, F0, rtol=1e-10, max_it=5000, history=True)
    assert info["converged"] == 1 and info0["converged"] == 1
    assert abs(info["iterations"] - info0["iterations"]) <= 2
    h = fs.residual_history()
    k = min(len(h), len(info0["history"]), 60)
    np.testing.assert_allclose(h[:k], info0["history"][:k], rtol=1e-6)
    assert np.linalg.norm(u.ravel() - u0) <= 1e-9 * np.linalg.norm(u0)


def test_single_reduction_recurrence_matches_classic_and_oracle(monkeypatch):
    # the recurrence multi-rank solves use (Chronopoulos-Gear: r.z, r.r, z.Az reduced together), forced on one rank
    m = meshes.structured(24, 20, 0, 0, 10, 8, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    m.xyz[:, 2] = 0.3 * np.sin(0.5 * m.xyz[:, 0]) * np.cos(0.4 * m.xyz[:, 1])
    fs = make_ctx(m, 0.3, 1e7, 0.5)
    u0, info0 = fs.solve(rtol=1e-11, max_it=20000)
    h0 = fs.residual_history()
    monkeypatch.setenv("FEMSHELL_CG_SINGLE_REDUCTION", "1")
    u1, info1 = fs.solve(rtol=1e-11, max_it=20000)
    h1 = fs.residual_history()
    monkeypatch.delenv("FEMSHELL_CG_SINGLE_REDUCTION")
    assert info0["converged"] == 1 and info1["converged"] == 1
    assert abs(info0["iterations"] - info1["iterations"]) <= 2
    k = min(len(h0), len(h1), 80)
    np.testing.assert_allclose(h1[:k], h0[:k], rtol=1e-6)
    assert np.linalg.norm(u1 - u0) <= 1e-9 * np.linalg.norm(u0)
    assert 0 <= info1["true_rel_residual"] < 1e-9
    mat = oracle.material(0.3, 1e7, 0.5)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), m.loads)
    uo, infoo = oracle.pcg(r0, c0, v0, F0, rtol=1e-11, max_it=20000)
    assert np.linalg.norm(u1.ravel() - uo) <= 1e-8 * np.linalg.norm(uo)
    # rtol = 0 runs exactly max_it iterations here as well
    monkeypatch.setenv("FEMSHELL_CG_SINGLE_REDUCTION", "1")
    _, info2 = fs.solve(rtol=0.0, max_it=37)
    assert info2["iterations"] == 37 and info2["converged"] == 0


def test_folded_single_reduction_iteration_is_bitwise_the_unfolded_one(monkeypatch):
    # multi-rank iteration: the scalar step and the collection of the transposed products are folded into the update
    # kernel (four kernels + one all-reduce per iteration); FEMSHELL_CG_FOLD=0 keeps them as launches of their own
    m = curved_mesh(30, 22)
    fs = make_ctx(m, 0.3, 7.0e4, 0.05)
    monkeypatch.setenv("FEMSHELL_CG_SINGLE_REDUCTION", "1")
    out = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("FEMSHELL_CG_FOLD", fold)
        u, info = fs.solve(rtol=1e-11, max_it=40000)
        uf, infof = fs.solve(rtol=0.0, max_it=53)
        out[fold] = (u, info, fs.residual_history(), uf, infof)
    monkeypatch.delenv("FEMSHELL_CG_FOLD")
    monkeypatch.delenv("FEMSHELL_CG_SINGLE_REDUCTION")
    (u1, i1, h1, uf1, if1), (u0, i0, h0, uf0, if0) = out["1"], out["0"]
    assert i1["converged"] == 1 and i0["converged"] == 1 and i1["iterations"] == i0["iterations"]
    assert if1["iterations"] == 53 and if0["iterations"] == 53
    assert np.array_equal(u1, u0) and np.array_equal(uf1, uf0) and np.array_equal(h1, h0)
    assert 0 <= i1["true_rel_residual"] < 1e-9


def test_fixed_iteration_mode_and_resolve_with_new_loads():
    m = curved_mesh(24, 18)
    fs = make_ctx(m, 0.3, 7.0e4, 0.05)
    _, info = fs.solve(rtol=0.0, max_it=37, fetch=False)
    assert info["iterations"] == 37 and info["converged"] == 0
    # linearity: solving with 2x the loads gives 2x the displacements (K, preconditioner reused)
    u1, i1 = fs.solve(rtol=1e-12, max_it=40000)
    fs.set_loads(2.0 * m.loads)
    u2, i2 = fs.solve(rtol=1e-12, max_it=40000)
    assert i2["assemble_seconds"] == 0.0
    assert np.linalg.norm(u2 - 2.0 * u1) <= 1e-9 * np.linalg.norm(u2)


# ------------------------------------------------------------------ size-independent properties at scale

def test_large_mesh_properties():
    # 512x512 squares -> 524,288 triangles, 263,169 nodes (config-2 class size)
    nx = 512
    m = meshes.structured(nx, nx, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    fs = make_ctx(m, 0.3, 1e7, 0.5, with_bc=False)
    fs.assemble()
    rng = np.random.default_rng(7)
    x = rng.normal(size=6 * m.n_nodes)
    y = rng.normal(size=6 * m.n_nodes)
    Kx, Ky = fs.spmv(x), fs.spmv(y)
    # symmetry: y.Kx == x.Ky
    assert abs(y @ Kx - x @ Ky) <= 1e-11 * (np.linalg.norm(y) * np.linalg.norm(Kx))
    # rigid-body translations and an in-plane rotation produce no force without constraints
    scale = np.linalg.norm(Kx) / np.linalg.norm(x)
    for mode in range(3):
        v = np.zeros((m.n_nodes, 6))
        v[:, mode] = 1.0
        assert np.linalg.norm(fs.spmv(v.ravel())) <= 1e-9 * scale * np.sqrt(m.n_nodes)
    v = np.zeros((m.n_nodes, 6))
    # rotation about z; the drilling dof is an uncoupled penalty (SA:1035-1052), so it stays 0
    v[:, 0], v[:, 1] = -m.xyz[:, 1], m.xyz[:, 0]
    assert np.linalg.norm(fs.spmv(v.ravel())) <= 1e-8 * scale * np.linalg.norm(v)
    # with supports: CG residual drops monotonically-ish and the solve is repeatable bit for bit
    fs.set_dirichlet(m.dirichlet_mask())
    u1, i1 = fs.solve(rtol=0.0, max_it=200)
    u2, i2 = fs.solve(rtol=0.0, max_it=200)
    assert np.array_equal(u1, u2)
    h = fs.residual_history()
    assert len(h) == 200 and np.isfinite(h).all()


def test_rccl_can_be_loaded_on_the_gpu_box():
    # the multi-rank path opens librccl lazily; make sure that works where the GPUs are
    uid = pkg.comm_unique_id()
    assert uid.shape == (128,) and uid.any()
    fs = pkg.FemShell(0.3, 1.0, 1.0, rank=0, world_size=1)
    fs.comm_init(uid)  # no-op for one rank
    assert fs.comm_selftest() is None  # (no communicator, nothing to test)


def test_solve_through_a_one_rank_rccl_communicator(monkeypatch):
    # the all-reduce / gather calls of the multi-rank driver, on the one GPU a test box has
    monkeypatch.setenv("FEMSHELL_FORCE_COMM", "1")
    m = meshes.load_example("test_C_w_tA16")
    fs = pkg.FemShell(0.3, 10.92, 1.0, rank=0, world_size=1)
    fs.comm_init(pkg.comm_unique_id())
    # first contact: femshell_comm_init ran the patterns of a solve once each with a known answer (real librccl, one rank:
    # all-reduce on the main stream, grouped broadcast; the send/recv ring needs a second rank -- tests/test_multirank_gpu.py)
    st = fs.comm_selftest()
    assert st is not None and all(v > 0.0 for v in st.values()), st
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    # a context with a communicator defaults to the single-reduction recurrence (all-reduce of three sums)
    u, info = fs.solve(rtol=1e-12, max_it=20000)
    assert info["converged"] == 1
    assert u[144, 2] == pytest.approx(1.15169, abs=6e-6)
    # the classic recurrence through the communicator (all-reduces of one and two sums)
    monkeypatch.setenv("FEMSHELL_CG_SINGLE_REDUCTION", "0")
    uc, infoc = fs.solve(rtol=1e-12, max_it=20000)
    monkeypatch.delenv("FEMSHELL_CG_SINGLE_REDUCTION")
    monkeypatch.delenv("FEMSHELL_FORCE_COMM")
    fs2 = make_ctx(m, 0.3, 10.92, 1.0)
    u2, info2 = fs2.solve(rtol=1e-12, max_it=20000)
    assert infoc["iterations"] == info2["iterations"]
    assert np.array_equal(uc, u2)  # a one-rank all-reduce changes nothing
    assert abs(info["iterations"] - info2["iterations"]) <= 3
    assert np.linalg.norm(u - u2) <= 1e-9 * np.linalg.norm(u2)


# ------------------------------------------------------------------ error behaviour

def test_errors_are_reported_not_swallowed():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], dtype=np.float64)
    tri = np.array([[0, 1, 2], [0, 1, 3]], dtype=np.int32)  # first triangle is collinear
    fs = pkg.FemShell(0.3, 1.0, 1.0)
    fs.set_mesh(xyz, tri)
    with pytest.raises(pkg.FemShellError) as ei:
        fs.assemble()
    assert ei.value.code == -4 and "triangle 0" in str(ei.value)
    with pytest.raises(pkg.FemShellError):
        pkg.FemShell(0.3, 1.0, 1.0).assemble()  # no mesh
    with pytest.raises(pkg.FemShellError):
        pkg.FemShell(0.3, -1.0, 1.0)
    fs2 = pkg.FemShell(0.3, 1.0, 1.0)
    with pytest.raises(pkg.FemShellError):
        fs2.set_mesh(xyz, np.array([[0, 1, 7]], dtype=np.int32))


# ------------------------------------------------------------------ BASELINE.json configurations (scaled down)

def _solve_and_compare(m, nu, E, t, rtol=1e-13, tol_solver=1e-9, tol_total=1e-7, max_it=200000):
    """Displacement parity, split into its two sources:
      solver error  |u_gpu - Kgpu^-1 F| / |u|: the CG result against an extended-precision-refined direct
                    solve of the matrix the GPU assembled (exported) -- must be < 1e-9 (measured 5e-15 ... 2.5e-10;
                    the accuracy CG can attain is kappa*eps, about 1e-8 on the 1k-element cantilever);
      total error   |u_gpu - Koracle^-1 F| / |u|: additionally contains kappa(K) * (rounding differences of
                    the two assembled matrices, <= 1e-12 relative, different summation order / FMA).  On
                    ill-conditioned shells (kappa ~ 1e8 on the 1k-element cantilever) this term alone is
                    ~1e-8, for ANY solver -- the reference's own PETSc solve included -- so the total is
                    only bounded loosely here and the matrix parity is asserted separately."""
    fs = make_ctx(m, nu, E, t)
    u, info = fs.solve(rtol=rtol, max_it=max_it)
    mat = oracle.material(nu, E, t)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), m.loads)
    rg, cg, vg, Fg = fs.export_bsr()
    assert np.abs(vg - v0).max() <= 1e-12 * np.abs(v0).max()
    u_gpu_matrix = oracle.refined_solve(rg, cg, vg, Fg)
    u_oracle_matrix = oracle.refined_solve(r0, c0, v0, F0)
    nrm = np.linalg.norm(u_oracle_matrix)
    err_solver = np.linalg.norm(u.ravel() - u_gpu_matrix) / nrm
    err_total = np.linalg.norm(u.ravel() - u_oracle_matrix) / nrm
    sens = np.linalg.norm(u_gpu_matrix - u_oracle_matrix) / nrm
    print("iterations %d, solver error %.2e, total error %.2e (matrix-rounding sensitivity %.2e)"
          % (info["iterations"], err_solver, err_total, sens))
    assert info["converged"] == 1
    true_res = np.linalg.norm(Fg - oracle.spmv(rg, cg, vg, u.ravel())) / np.linalg.norm(Fg)
    # the device's own explicit b - K u: same value up to the rounding of the residual evaluation itself
    assert 0.2 * true_res <= info["true_rel_residual"] <= 5.0 * true_res or max(true_res, info["true_rel_residual"]) < 1e-11
    assert err_solver < tol_solver, err_solver
    assert err_total < tol_total, err_total
    return u, info


@pytest.mark.parametrize("ul_lr", [True, False])
def test_config1_cantilever_1k_tri_tip_load(ul_lr):
    # BASELINE configs[0]: cantilever 48x12, 32x16 squares -> 1024 tri3, left edge clamped (id 1), tip load
    m = meshes.structured(32, 16, 0, 0, 48, 12, kind="t", ul_lr=ul_lr, bcids=(-1, -1, 1, -1))
    tip = 8 * 33 + 32
    m.loads[tip, 2] = 1.0        # bending
    m.loads[tip, 1] = 40.0       # in-plane shear, Test-A style
    u, info = _solve_and_compare(m, 0.25, 30000.0, 1.0)
    assert u[tip, 2] > 0 and u[tip, 1] > 0


def test_config2_scordelis_lo_roof_scaled():
    # BASELINE configs[1] at 40x40 squares (3200 tri3); the full 354x354 case runs in bench.py --workload roof
    m = meshes.scordelis_lo(40)
    nu, E, t = m.material
    _solve_and_compare(m, nu, E, t)


def test_config3_pinched_cylinder_scaled():
    # BASELINE configs[2] at 64 x 32 squares (periodic in theta)
    m = meshes.pinched_cylinder(64, 32)
    nu, E, t = m.material
    u, _ = _solve_and_compare(m, nu, E, t)
    mid = 16 * 64
    assert u[mid, 0] < 0 < u[mid + 32, 0]  # both load points move inwards
    assert abs(u[mid, 0] + u[mid + 32, 0]) <= 1e-9 * abs(u[mid, 0])  # symmetry of the pinch


# ------------------------------------------------------------------ unstructured meshes (irregular valence)

def delaunay_shell(n_pts, seed, jittered=False):
    """Random Delaunay triangulation of a curved patch, node numbering shuffled: valences 3..10+, so slices
    are wide and ragged, gather lists are uneven and many slices need several assembly rounds."""
    from scipy.spatial import Delaunay

    rng = np.random.default_rng(seed)
    if jittered:  # a grid with every interior point moved by up to 0.35 spacings: irregular valence, no slivers
        side = int(np.sqrt(n_pts))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float64)
        inner = np.all((g > 0) & (g < side - 1), axis=1)[:, None]  # the boundary stays straight: no hull slivers
        uv = (g + inner * rng.uniform(-0.35, 0.35, size=g.shape)) / (side - 1)
        n_pts = len(uv)
    else:
        uv = rng.uniform(0.0, 1.0, size=(n_pts, 2))
    tri = Delaunay(uv).simplices.astype(np.int32)
    # drop slivers on the hull (nearly collinear points)
    p, q, r = uv[tri[:, 0]], uv[tri[:, 1]], uv[tri[:, 2]]
    area = 0.5 * np.abs((q[:, 0] - p[:, 0]) * (r[:, 1] - p[:, 1]) - (q[:, 1] - p[:, 1]) * (r[:, 0] - p[:, 0]))
    tri = tri[area > (0.05 * area.mean() if jittered else 1e-7)]
    used = np.unique(tri)
    remap = -np.ones(n_pts, dtype=np.int64)
    remap[used] = rng.permutation(len(used))
    tri = remap[tri].astype(np.int32)
    uv2 = np.zeros((len(used), 2))
    uv2[remap[used]] = uv[used]
    xyz = np.stack([3.0 * uv2[:, 0], 2.0 * uv2[:, 1], 0.3 * np.sin(3.0 * uv2[:, 0]) * np.cos(2.0 * uv2[:, 1])], axis=1)
    return xyz, tri


@pytest.mark.parametrize("n_pts,seed", [(700, 1), (3000, 2)])
def test_unstructured_delaunay_shell(n_pts, seed):
    xyz, tri = delaunay_shell(n_pts, seed)
    n = len(xyz)
    rng = np.random.default_rng(seed)
    dmask = np.zeros(n, dtype=np.uint8)
    dmask[xyz[:, 0] < 0.15] = 0x3F          # clamp one side
    dmask[rng.integers(0, n, 5)] |= 0x07    # a few pinned points
    loads = rng.normal(size=(n, 6))
    fs = pkg.FemShell(0.3, 7.0e4, 0.03)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.assemble()
    rg, cg, vg, Fg = fs.export_bsr()
    mat = oracle.material(0.3, 7.0e4, 0.03)
    r0, c0, v0, F0 = oracle.assemble(xyz, tri, np.zeros((0, 4), np.int32), mat, dmask, loads)
    np.testing.assert_array_equal(rg, r0)
    np.testing.assert_array_equal(cg, c0)
    assert np.abs(vg - v0).max() <= 1e-12 * np.abs(v0).max()
    np.testing.assert_array_equal(Fg, F0)
    x = rng.normal(size=6 * n)
    # the product kernel against the same matrix (1e-13), and against the oracle's matrix (the assembly's 1e-12 enters)
    y_ref = oracle.spmv(r0, c0, v0, x)
    assert np.linalg.norm(fs.spmv(x) - oracle.spmv(rg, cg, vg, x)) <= 1e-13 * np.linalg.norm(y_ref)
    assert np.linalg.norm(fs.spmv(x) - y_ref) <= 1e-12 * np.linalg.norm(y_ref)
    # slivers on the hull make these systems so ill-conditioned that block-Jacobi CG stagnates around 1e-9
    # (the CPU oracle does too, after 300k iterations), so: (1) the two solvers are compared iteration by
    # iteration (finite-precision CG is chaotic here: the histories agree to 1e-9 at first and drift apart later),
    # (2) a moderately converged solve is checked against a refined direct solve of the same matrix
    _, info = fs.solve(rtol=0.0, max_it=200, fetch=False)
    _, info0 = oracle.pcg(r0, c0, v0, F0, rtol=0.0, max_it=200, history=True)
    h = fs.residual_history()
    assert len(h) == 200
    np.testing.assert_allclose(h[:30], info0["history"][:30], rtol=1e-6)
    if n_pts <= 1000:
        u, info = fs.solve(rtol=1e-8, max_it=60000)
        assert info["converged"] == 1
        u_ref = oracle.refined_solve(rg, cg, vg, Fg)
        assert np.linalg.norm(u.ravel() - u_ref) <= 1e-5 * np.linalg.norm(u_ref)
        assert 0.0 < info["true_rel_residual"] <= 1e-4  # drifts two orders above the recurrence residual here


def test_tiny_meshes():
    # one triangle, one quad, fewer nodes than a slice
    for xyz, tri, quad in (
        (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], dtype=np.float64), np.array([[0, 1, 2]], np.int32), None),
        (np.array([[0, 0, 0], [2, 0, 0], [2, 1, 0], [0, 1, 0]], dtype=np.float64), None, np.array([[0, 1, 2, 3]], np.int32)),
    ):
        fs = pkg.FemShell(0.3, 1000.0, 0.1)
        fs.set_mesh(xyz, tri, quad)
        dmask = np.zeros(len(xyz), dtype=np.uint8)
        dmask[0] = 0x3F
        dmask[1] = 0x3F
        fs.set_dirichlet(dmask)
        loads = np.zeros((len(xyz), 6))
        loads[-1, 2] = 1.0
        fs.set_loads(loads)
        u, info = fs.solve(rtol=1e-13, max_it=1000)
        mat = oracle.material(0.3, 1000.0, 0.1)
        t_ = np.zeros((0, 3), np.int32) if tri is None else tri
        q_ = np.zeros((0, 4), np.int32) if quad is None else quad
        r0, c0, v0, F0 = oracle.assemble(xyz, t_, q_, mat, dmask, loads)
        u0 = oracle.direct_solve(r0, c0, v0, F0)
        assert info["converged"] == 1
        assert np.linalg.norm(u.ravel() - u0) <= 1e-10 * np.linalg.norm(u0)


def test_context_reuse_new_mesh_new_constraints():
    """One context, used the way a long-running program would: a mesh, a solve, a different (larger, mixed) mesh on
    the same context, a change of the Dirichlet set after assembly, a change of the loads only; every state must
    equal what a fresh context computes."""
    def fresh(m, nu, E, t, dmask, loads):
        fs_ = pkg.FemShell(nu, E, t)
        fs_.set_mesh(m.xyz, m.tri, m.quad)
        fs_.set_dirichlet(dmask)
        fs_.set_loads(loads)
        u_, info_ = fs_.solve(rtol=1e-12, max_it=100000)
        assert info_["converged"] == 1
        return u_, fs_.export_bsr()

    rng = np.random.default_rng(3)
    a = meshes.structured(9, 7, 0, 0, 3, 2, kind="t", ul_lr=True, bcids=(0, -1, 1, -1), factor=2.0, loading=2)
    b = meshes.structured(37, 41, 0, 0, 5, 6, kind="q", bcids=(1, -1, -1, 0), factor=1.0, loading=2)
    fs = pkg.FemShell(0.3, 2.0e5, 0.05)
    for m in (a, b, a):  # smaller -> larger -> smaller again: every device buffer is re-sized both ways
        dmask, loads = m.dirichlet_mask(), m.loads
        fs.set_mesh(m.xyz, m.tri, m.quad)
        fs.set_dirichlet(dmask)
        fs.set_loads(loads)
        u, info = fs.solve(rtol=1e-12, max_it=100000)
        u_ref, (r0, c0, v0, F0) = fresh(m, 0.3, 2.0e5, 0.05, dmask, loads)
        assert info["converged"] == 1
        np.testing.assert_array_equal(u, u_ref)  # same kernels, same data: bitwise
        # new Dirichlet set on the assembled context (constraint words, K, F and the Jacobi blocks must follow)
        dmask2 = dmask.copy()
        dmask2[rng.integers(0, m.n_nodes, 4)] |= 0x15
        fs.set_dirichlet(dmask2)
        u2, _ = fs.solve(rtol=1e-12, max_it=100000)
        u2_ref, (r2, c2, v2, F2) = fresh(m, 0.3, 2.0e5, 0.05, dmask2, loads)
        np.testing.assert_array_equal(u2, u2_ref)
        rg, cg, vg, Fg = fs.export_bsr()
        np.testing.assert_array_equal(vg, v2)
        np.testing.assert_array_equal(Fg, F2)
        # new loads only: K is kept, the right-hand side is rebuilt
        loads3 = rng.normal(size=loads.shape)
        fs.set_loads(loads3)
        u3, info3 = fs.solve(rtol=1e-12, max_it=100000)
        u3_ref, _ = fresh(m, 0.3, 2.0e5, 0.05, dmask2, loads3)
        assert info3["assemble_seconds"] == 0.0
        np.testing.assert_array_equal(u3, u3_ref)


# ------------------------------------------------------------------ symmetric storage against full storage

def test_symmetric_storage_equals_full_storage(monkeypatch):
    """K is stored as diagonal + one block per pair of owned nodes (default) or in full (FEMSHELL_SYMMETRIC=0, the
    round-1 layout): same matrix up to the 1e-16 by which the reference's two independently summed blocks of a pair
    differ, same products to 1e-13, same solve; products and solves are bitwise reproducible in both layouts."""
    m = curved_mesh(41, 33)
    rng = np.random.default_rng(11)
    x = rng.normal(size=6 * m.n_nodes)
    out = {}
    for sym in ("1", "0"):
        monkeypatch.setenv("FEMSHELL_SYMMETRIC", sym)
        fs = make_ctx(m, 0.3, 7.0e4, 0.05)
        fs.assemble()
        r, c, v, F = fs.export_bsr()
        y1, y2 = fs.spmv(x), fs.spmv(x)
        assert np.array_equal(y1, y2)
        u1, i1 = fs.solve(rtol=1e-11, max_it=50000)
        u2, i2 = fs.solve(rtol=1e-11, max_it=50000)
        assert np.array_equal(u1, u2) and i1["iterations"] == i2["iterations"] and i1["converged"] == 1
        out[sym] = (r, c, v, F, y1, u1, i1, fs.residual(u1))
        fs.close()
    monkeypatch.delenv("FEMSHELL_SYMMETRIC")
    (r1, c1, v1, F1, y1, u1, i1, res1), (r0, c0, v0, F0, y0, u0, i0, res0) = out["1"], out["0"]
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(F1, F0)
    assert np.abs(v1 - v0).max() <= 1e-14 * np.abs(v0).max()
    # exactly symmetric outside the diagonal blocks with symmetric storage (a diagonal block is a sum of element blocks
    # that are symmetric to rounding only, like the reference's)
    K1 = oracle.to_scipy(r1, c1, v1)
    D = (K1 - K1.T).tocoo()
    off = (D.row // 6) != (D.col // 6)
    assert np.abs(D.data[off]).max(initial=0.0) == 0.0
    assert np.abs(D.data).max(initial=0.0) <= 1e-14 * abs(K1).max()
    assert np.linalg.norm(y1 - y0) <= 1e-13 * np.linalg.norm(y0)
    assert abs(i1["iterations"] - i0["iterations"]) <= max(3, 0.02 * i0["iterations"])
    assert np.linalg.norm(u1 - u0) <= 1e-8 * np.linalg.norm(u0)
    # the double-double residuals of the two layouts agree far below the FP64 noise of either
    assert np.linalg.norm(res1 - oracle_residual(r1, c1, v1, F1, u1)) <= 1e-11 * np.linalg.norm(F1)
    assert np.linalg.norm(res0 - oracle_residual(r0, c0, v0, F0, u0)) <= 1e-11 * np.linalg.norm(F0)


def test_products_kept_in_the_slice_equal_the_products_through_hbm(monkeypatch):
    """A stored block (a, c) with c in a's own slice hands K_ac^T x_a to row c through LDS (default) or, with
    FEMSHELL_SPMV_LOCAL=0, through HBM like every other transposed product: the same product to rounding (the sums of a
    row take another order), both equal to the oracle's, each reproducible bit by bit, and the same solve."""
    cases = [curved_mesh(41, 33), meshes.structured(37, 29, 0, 0, 3, 2, kind="q", bcids=(0, 0, 1, -1), factor=3.0, loading=2)]
    xyz, tri = delaunay_shell(2500, 7)
    for m in cases + [None]:
        if m is None:
            n, X, T, Q = len(xyz), xyz, tri, np.zeros((0, 4), np.int32)
            dm = np.zeros(n, dtype=np.uint8); dm[X[:, 0] < 0.2] = 0x3F
            ld = np.zeros((n, 6)); ld[:, 2] = 1.0
        else:
            n, X, T, Q, dm, ld = m.n_nodes, m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads
        x = np.random.default_rng(2).normal(size=6 * n)
        out = {}
        for loc in ("1", "0"):
            monkeypatch.setenv("FEMSHELL_SPMV_LOCAL", loc)
            fs = pkg.FemShell(0.3, 7.0e4, 0.05)
            fs.set_mesh(X, T, Q); fs.set_dirichlet(dm); fs.set_loads(ld); fs.assemble()
            y1, y2 = fs.spmv(x), fs.spmv(x)
            assert np.array_equal(y1, y2)
            u, its = None, 0
            if m is cases[0]:  # (the solve on the triangle mesh only: block-Jacobi CG is slow on the other two)
                u, info = fs.solve(rtol=1e-11, max_it=100000)
                assert info["converged"] == 1
                its = info["iterations"]
            r, c, v, F = fs.export_bsr()
            out[loc] = (y1, u, its)
            fs.close()
        monkeypatch.delenv("FEMSHELL_SPMV_LOCAL")
        y0 = oracle.spmv(r, c, v, x)
        scale = np.abs(v).max() * np.abs(x).max()
        assert np.abs(out["1"][0] - y0).max() <= 1e-13 * scale and np.abs(out["0"][0] - y0).max() <= 1e-13 * scale
        assert not np.array_equal(out["1"][0], out["0"][0]) or len(T) == 0  # (the knob did something)
        if m is cases[0]:
            assert abs(out["1"][2] - out["0"][2]) <= max(3, 0.02 * out["0"][2])
            assert np.linalg.norm(out["1"][1] - out["0"][1]) <= 1e-8 * np.linalg.norm(out["0"][1])


def oracle_residual(r, c, v, F, u):
    K = oracle.to_scipy(r, c, v)
    K.sort_indices()
    ld = np.longdouble
    return (F.astype(ld) - np.add.reduceat(K.data.astype(ld) * u.ravel().astype(ld)[K.indices], K.indptr[:-1])).astype(np.float64)


@pytest.mark.parametrize("flag", ["REORDER_MORTON", "REORDER_RCM"])
def test_internal_renumbering_is_invisible_at_the_boundary(flag):
    """FEMSHELL_REORDER_MORTON / _RCM renumber the nodes inside the library only (csrc/reorder.cpp): on a Delaunay mesh
    with shuffled numbering every node-indexed argument and result keeps the caller's ids -- the exported matrix, right
    hand side, products, residuals, element matrices and the solution equal those of a context without the flag (and
    the oracle's), sparse Dirichlet / load lists included; both preconditioners."""
    xyz, tri = delaunay_shell(2500, 5, jittered=True)
    n = len(xyz)
    rng = np.random.default_rng(3)
    fixed = np.flatnonzero(xyz[:, 0] < 0.2).astype(np.int32)
    loaded = rng.choice(n, 40, replace=False).astype(np.int32)
    f6 = rng.normal(size=(40, 6))
    x = rng.normal(size=6 * n)
    res = {}
    for name, flags in (("plain", pkg.REF_DEFAULT), ("reordered", pkg.REF_DEFAULT | getattr(pkg, flag))):
        fs = pkg.FemShell(0.3, 7.0e4, 0.03, flags=flags)
        fs.set_mesh(xyz, tri)
        fs.set_dirichlet(np.full(len(fixed), 0x3F, np.uint8), node_ids=fixed)
        fs.set_loads(f6, node_ids=loaded)
        fs.assemble()
        r, c, v, F = fs.export_bsr()
        y = fs.spmv(x)
        ke = fs.element_matrices(0, 50)
        fs.set_preconditioner("amg")
        u_amg, i_amg = fs.solve(rtol=1e-12, max_it=500)
        assert i_amg["converged"] == 1
        rr = fs.residual(u_amg)
        fs.set_preconditioner("block_jacobi")
        _, i_bj = fs.solve(rtol=0.0, max_it=60, fetch=False)
        res[name] = (r, c, v, F, y, ke, u_amg, rr, fs.residual_history())
        fs.close()
    (r0, c0, v0, F0, y0, ke0, u0, rr0, h0), (r1, c1, v1, F1, y1, ke1, u1, rr1, h1) = res["plain"], res["reordered"]
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(F1, F0)
    np.testing.assert_array_equal(ke1, ke0)
    assert np.abs(v1 - v0).max() <= 1e-13 * np.abs(v0).max()   # same element sums in another order
    assert np.linalg.norm(y1 - y0) <= 1e-13 * np.linalg.norm(y0)
    np.testing.assert_allclose(h1[:20], h0[:20], rtol=1e-6)     # same block-Jacobi CG, iteration by iteration
    dmask = np.zeros(n, np.uint8)
    dmask[fixed] = 0x3F
    loads = np.zeros((n, 6))
    loads[loaded] = f6
    ro, co, vo, Fo = oracle.assemble(xyz, tri, np.zeros((0, 4), np.int32), oracle.material(0.3, 7.0e4, 0.03), dmask, loads)
    np.testing.assert_array_equal(r1, ro)
    np.testing.assert_array_equal(c1, co)
    np.testing.assert_array_equal(F1, Fo)
    assert np.abs(v1 - vo).max() <= 1e-12 * np.abs(vo).max()
    # both solutions solve their own (rounding-different) matrices to the refinement floor; they agree to kappa * eps
    assert np.linalg.norm(rr1) <= 1e-10 * np.linalg.norm(F1)
    assert np.linalg.norm(rr1 - oracle_residual(r1, c1, v1, F1, u1)) <= 1e-11 * np.linalg.norm(F1)
    assert np.linalg.norm(u1 - u0) <= 1e-6 * np.linalg.norm(u0)
    assert np.all(u1[fixed] == 0.0)


def _fan_mesh():
    m = meshes.structured(20, 20, 0, 0, 2, 2, kind="t", ul_lr=True)
    ang = np.linspace(0.0, 2.0 * np.pi, 41)[:-1]
    hub = len(m.xyz)
    ring = np.stack([3.0 + 0.5 * np.cos(ang), 1.0 + 0.5 * np.sin(ang), np.zeros(40)], axis=1)
    xyz = np.concatenate([m.xyz, [[3.0, 1.0, 0.2]], ring])
    fan = np.array([[hub, hub + 1 + k, hub + 1 + (k + 1) % 40] for k in range(40)], dtype=np.int32)
    return xyz, np.concatenate([m.tri, fan]).astype(np.int32)


@pytest.mark.parametrize("mesh", ["panel", "patch", "hub", "quads", "mixed"])
@pytest.mark.parametrize("symmetric", ["1", "0"])
def test_pipelined_and_two_phase_assembly_kernels_agree(monkeypatch, mesh, symmetric):
    """k_assemble_pipe (producer wave + three consumer waves, records as a stream across slices, partial sums through lane
    shifts) against k_assemble (records, barrier, blocks) and against the oracle: structured panel, Delaunay patch with
    valences 3..12 (slots of one to four chunks, mixed waves, several rounds), a fan of 40 triangles around one node (a
    slot of 14 chunks), quadrilaterals and a mix of both element types (66-double records, every block through the
    general block function); Dirichlet rows and columns, right-hand side; symmetric and full storage."""
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", symmetric)
    if mesh == "panel":
        m = meshes.structured(70, 45, 0, 0, 7, 4.5, kind="t", ul_lr=True)
        xyz, tri = m.xyz.copy(), m.tri
        xyz[:, 2] = 0.3 * np.sin(0.9 * xyz[:, 0]) * np.cos(0.7 * xyz[:, 1])
    elif mesh == "patch":
        xyz, tri = meshes.delaunay_patch(3000, 7)
    elif mesh == "hub":
        xyz, tri = _fan_mesh()
    quad = np.zeros((0, 4), np.int32)
    if mesh in ("quads", "mixed"):  # planar quadrilaterals, tilted; "mixed": every eighth one cut into two triangles (a
        # slice may touch 77 elements at most when their records are the 66-double ones)
        m = meshes.structured(40, 30, 0, 0, 4.0, 3.3, kind="q")
        qm, _ = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))
        xyz, quad = m.xyz @ qm.T, m.quad.copy()
        tri = np.zeros((0, 3), np.int32)
        if mesh == "mixed":
            pick = np.arange(len(quad)) % 8 == 0
            q = quad[pick]
            tri = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]]).astype(np.int32)
            quad = quad[~pick]
    n = len(xyz)
    rng = np.random.default_rng(12)
    dmask = np.zeros(n, np.uint8)
    dmask[rng.choice(n, n // 9, replace=False)] = rng.integers(1, 64, n // 9).astype(np.uint8)
    loads = rng.normal(size=(n, 6))
    out = {}
    for pipe in ("1", "0"):
        monkeypatch.setenv("FEMSHELL_ASM_PIPE", "2" if pipe == "1" else "0")  # 2: wherever the pipelined kernel can run
        assert pkg.build_plan(xyz, tri, quad)["pipe"] == int(pipe)
        fs = pkg.FemShell(0.3, 2.1e5, 0.04)
        fs.set_mesh(xyz, tri, quad)
        assert fs.assembly_kernel() == ("k_assemble_pipe" if pipe == "1" else "k_assemble")
        fs.set_dirichlet(dmask)
        fs.set_loads(loads)
        fs.assemble()
        out[pipe] = fs.export_bsr()
        out[pipe + "again"] = fs.export_bsr() if pipe == "0" else None
        if pipe == "1":  # run to run: the same bits
            fs.assemble()
            r2, c2, v2, F2 = fs.export_bsr()
            np.testing.assert_array_equal(v2, out["1"][2])
        fs.close()
    (r1, c1, v1, F1), (r0, c0, v0, F0) = out["1"], out["0"]
    np.testing.assert_array_equal(r1, r0)
    np.testing.assert_array_equal(c1, c0)
    np.testing.assert_array_equal(F1, F0)
    assert np.abs(v1 - v0).max() <= 1e-13 * np.abs(v0).max()
    ro, co, vo, Fo = oracle.assemble(xyz, tri, quad, oracle.material(0.3, 2.1e5, 0.04), dmask, loads)
    np.testing.assert_array_equal(r1, ro)
    np.testing.assert_array_equal(c1, co)
    np.testing.assert_array_equal(F1, Fo)
    assert np.abs(v1 - vo).max() <= 1e-12 * np.abs(vo).max()


def test_asynchronous_assembly_reports_its_status_at_the_next_synchronising_call():
    """femshell_assemble_async enqueues the assembly and returns; a degenerate element is reported by the next call that
    synchronises, reads K or changes the inputs -- and the context works on after the mesh is repaired.  A good mesh gives
    the bits of the synchronous call."""
    m = meshes.structured(24, 18, 0, 0, 4, 3, kind="t", ul_lr=True, bcids=(0, 0, 1, -1), factor=2.0, loading=2)
    fs = pkg.FemShell(0.3, 1e6, 0.1)
    fs.set_mesh(m.xyz, m.tri)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    fs.assemble()
    ref = fs.export_bsr()
    for _ in range(3):
        fs.assemble(wait=False)
    fs.sync()
    got = fs.export_bsr()
    for a, b in zip(ref, got):
        np.testing.assert_array_equal(a, b)
    u, info = fs.solve(rtol=1e-9, max_it=20000)
    assert info["converged"] == 1
    bad = m.xyz.copy()
    a, b, c = m.tri[37]
    bad[c] = bad[b]  # a triangle of zero area
    for how in ("sync", "solve", "export", "assemble", "set_loads"):
        fs.set_mesh(bad, m.tri)
        fs.set_dirichlet(m.dirichlet_mask())
        fs.set_loads(m.loads)
        fs.assemble(wait=False)  # returns: nothing has looked at the status yet
        with pytest.raises(pkg.FemShellError) as ei:
            {"sync": fs.sync, "solve": lambda: fs.solve(rtol=1e-6, max_it=10), "export": fs.export_bsr, "assemble": fs.assemble,
             "set_loads": lambda: fs.set_loads(m.loads)}[how]()
        assert ei.value.code == -4 and "degenerate" in str(ei.value), how  # FEMSHELL_ERR_MESH
    fs.set_mesh(m.xyz, m.tri)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    fs.assemble(wait=False)
    u2, info2 = fs.solve(rtol=1e-9, max_it=20000)
    assert info2["converged"] == 1 and np.array_equal(u2, u)
    fs.close()


def test_assembly_kernel_query():
    """femshell_assembly_kernel: an error before femshell_set_mesh, then the kernel the plan chose -- the pipelined one for
    a structured mesh, the two-phase one with FEMSHELL_ASM_PIPE=0 (read per femshell_set_mesh)."""
    m = meshes.structured(12, 9, 0, 0, 2, 1.5, kind="t", ul_lr=True)
    fs = pkg.FemShell(0.3, 1e6, 0.1)
    with pytest.raises(pkg.FemShellError) as ei:
        fs.assembly_kernel()
    assert ei.value.code == -1
    fs.set_mesh(m.xyz, m.tri)
    assert fs.assembly_kernel() == "k_assemble_pipe"
    os.environ["FEMSHELL_ASM_PIPE"] = "0"
    try:
        fs.set_mesh(m.xyz, m.tri)
        assert fs.assembly_kernel() == "k_assemble"
    finally:
        del os.environ["FEMSHELL_ASM_PIPE"]
    fs.close()
