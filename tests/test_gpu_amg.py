"""Multigrid-preconditioned solves on the GPU (csrc/amg_*.{cpp,hip}) against the CPU oracle: converged
displacements against the direct solve, the hierarchy against the numpy restatement oracle/amg_oracle.py,
iteration counts against the restatement's flexible PCG."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import amg_oracle
from tests.helpers import hierarchy, meshes, oracle
from tests.helpers.product import ensure_built, pkg

pytestmark = pytest.mark.gpu


def _make(kind, n):
    if kind == "panel":
        m = meshes.structured(n, n, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
        mat = (0.3, 1e7, 0.5)
    elif kind == "roof":
        m = meshes.scordelis_lo(n)
        mat = m.material
    elif kind == "cylinder":
        m = meshes.pinched_cylinder(n, n)
        mat = m.material
    elif kind == "quads":
        m = meshes.structured(n, n, 0, 0, 10, 10, kind="q", bcids=(1, 1, 1, 1), factor=300.0, loading=2)
        mat = (0.3, 1e7, 0.5)
    return m, mat


def _context(m, mat):
    ensure_built()
    fs = pkg.FemShell(*mat, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    return fs


def _bsr(rowptr, cols, vals, nc):
    n = len(rowptr) - 1
    return sp.bsr_matrix((vals, cols, rowptr), shape=(6 * n, 6 * nc))


@pytest.mark.parametrize("kind,n", [("panel", 64), ("roof", 48), ("cylinder", 48), ("quads", 40)])
def test_multigrid_solve_matches_the_direct_solve(kind, n):
    m, mat = _make(kind, n)
    fs = _context(m, mat)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=500)
    assert info["converged"] == 1 and info["pc_type"] == 1 and info["amg_levels"] >= 2
    rg, cg, vg, Fg = fs.export_bsr()
    # solver term: against the refined direct solve of the matrix the GPU assembled (north star: < 1e-10)
    ug = oracle.refined_solve(rg, cg, vg, Fg)
    err = np.linalg.norm(u.ravel() - ug) / np.linalg.norm(ug)
    assert err < 1e-10, err
    # block-Jacobi needs an order of magnitude more iterations on the same system
    fs.set_preconditioner("jacobi")
    u2, info2 = fs.solve(rtol=1e-12, max_it=200000)
    # (the multigrid count includes the refinement pass: about 40 % on top of the first phase)
    assert info2["converged"] == 1 and info2["iterations"] > 5 * info["iterations"], (info["iterations"], info2["iterations"])
    assert np.linalg.norm(u2.ravel() - ug) / np.linalg.norm(ug) < 2e-10
    fs.close()


@pytest.mark.parametrize("cycle", ["V", "K"])
def test_hierarchy_and_iteration_counts_follow_the_restatement(cycle):
    m, mat = _make("panel", 48)
    fs = _context(m, mat)
    fs.set_preconditioner("amg", cycle=cycle, coarsest_nodes=60)
    u, info = fs.solve(rtol=1e-10, max_it=400)
    assert info["converged"] == 1
    lv = fs.amg_levels()
    assert len(lv) >= 3 and lv[0]["n_nodes"] == m.n_nodes
    rg, cg, vg, Fg = fs.export_bsr()
    A = _bsr(rg, cg, vg, m.n_nodes)
    # the restatement with the library's spectral bounds (its power iteration starts from another vector): aggregates bit for bit,
    # P to 1e-11 and the level operators to 1e-10 of their largest entry, the bounds bracketed (tests/helpers/hierarchy.py)
    levels, got = hierarchy.compare(fs, m.xyz, m.dirichlet_mask(), m.tri, m.quad, coarsest_nodes=60)
    # (dependent columns of the tentative QR at the clamped corners: zero columns of P, unit diagonal entries of A_1)
    assert got["zero_columns"][0] == 6, got["zero_columns"]
    u0, hist = amg_oracle.solve(A, Fg, levels, kcycle=(cycle == "K"), rtol=1e-10, max_it=400, refine_passes=1)
    # (the counts of the two implementations differ by where their residuals cross the threshold: a few iterations, more
    # or fewer with the rounding of K -- 100 against 101..104 with the two assembly kernels)
    assert abs(len(hist) - info["iterations"]) <= 5, (len(hist), info["iterations"])
    h = fs.residual_history()
    k = min(len(h), len(hist), 20)
    np.testing.assert_allclose(h[:k], hist[:k], rtol=1e-5)
    assert np.linalg.norm(u.ravel() - u0) / np.linalg.norm(u0) < 1e-11
    fs.close()


@pytest.mark.parametrize("galerkin", ["valu", "mfma"])
def test_every_level_coarsened_on_the_device_follows_the_restatement_too(monkeypatch, galerkin):
    # level 0 and the levels above FEMSHELL_AMG_DEVICE_MIN nodes (5,000 by default: the test meshes seldom get there below
    # level 0) take their coarsening step with the numerics on the device; forced down to 100-node levels here.  Both Galerkin
    # kernels: one lane per result block on the vector ALUs (default) and one wave per coarse row on the matrix cores
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    monkeypatch.setenv("FEMSHELL_AMG_GALERKIN", galerkin)
    test_hierarchy_and_iteration_counts_follow_the_restatement("K")


def test_single_precision_smoothing_products_leave_the_solution_alone(monkeypatch):
    # FEMSHELL_AMG_SMOOTH_F32 (default 1: levels of at least 4096 nodes; 3: every level): the Chebyshev products read a float
    # copy of the level operators' values; the solve is flexible CG on the FP64 operator, so the answer is the same and the
    # iteration count moves by a few at most
    m, mat = _make("roof", 48)
    monkeypatch.setenv("FEMSHELL_AMG_SMOOTH_F32", "0")
    fs = _context(m, mat)
    fs.set_preconditioner("amg", coarsest_nodes=60)
    u, info = fs.solve(rtol=1e-12, max_it=500)
    fs.close()
    # FEMSHELL_AMG_VEC_F32: what such a product keeps in single precision besides the values -- 0 nothing, 1 its results (direct
    # part and transposed products), 2 (default) its input, the Chebyshev direction, as well
    seen = []
    for mode, vec in (("3", "2"), ("3", "1"), ("3", "0"), ("2", "2")):
        monkeypatch.setenv("FEMSHELL_AMG_SMOOTH_F32", mode)
        monkeypatch.setenv("FEMSHELL_AMG_VEC_F32", vec)
        fs = _context(m, mat)
        fs.set_preconditioner("amg", coarsest_nodes=60)
        u32, info32 = fs.solve(rtol=1e-12, max_it=500)
        assert info32["converged"] == 1 and info32["amg_levels"] >= 3
        assert abs(info32["iterations"] - info["iterations"]) <= 3, (mode, vec, info["iterations"], info32["iterations"])
        assert not np.array_equal(u32, u)  # (the knob did something)
        assert np.linalg.norm(u32 - u) / np.linalg.norm(u) < 1e-10
        assert all(not np.array_equal(u32, other) for other in seen)  # (... and every setting something of its own)
        seen.append(u32)
        fs.close()


@pytest.mark.parametrize("f32,vec", [("0", "0"), ("3", "2"), ("3", "1"), ("1", "2")])
def test_fused_smoother_starts_give_the_same_bits_as_the_separate_passes(monkeypatch, f32, vec):
    """FEMSHELL_AMG_FUSE (csrc/amg_solve.cpp): the first step of every Chebyshev smoothing runs in the epilogue of the kernel
    that produces its residual -- k_pcg_update_start_node on level 0 (bit 0), k_sym_gather_start_node in front of the post-smoothing of a
    symmetric-storage level (bit 1), the epilogue of k_spmv on a full-storage level (bit 2) -- instead of a k_cheb_start_node pass
    of its own.  The first two repeat the expressions of the kernels they replace: solution and iteration count are those of
    the unfused sequence bit for bit, on FP64 levels and on levels with single-precision copies.  The epilogue of k_spmv rounds
    x + c z differently from k_cheb_start_node (a contracted multiply-add): same iterations, solution equal to rounding."""
    m, mat = _make("roof", 64)
    monkeypatch.setenv("FEMSHELL_AMG_SMOOTH_F32", f32)
    monkeypatch.setenv("FEMSHELL_AMG_VEC_F32", vec)
    got = {}
    for fuse in ("0", "3", "-1"):
        monkeypatch.setenv("FEMSHELL_AMG_FUSE", fuse)
        fs = _context(m, mat)
        fs.set_preconditioner("amg", coarsest_nodes=60)
        u, info = fs.solve(rtol=1e-12, max_it=500)
        assert info["converged"] == 1 and info["amg_levels"] >= 3
        got[fuse] = (u, info["iterations"])
        fs.close()
    assert got["0"][1] == got["3"][1]
    np.testing.assert_array_equal(got["0"][0], got["3"][0])
    assert abs(got["0"][1] - got["-1"][1]) <= 1
    assert np.linalg.norm(got["0"][0] - got["-1"][0]) <= 1e-11 * np.linalg.norm(got["0"][0])


def test_inspection_copies_of_the_hierarchy_are_kept_for_small_problems_only(monkeypatch):
    # femshell_amg_export reads host copies of the level operators that the setup keeps for problems of up to 300,000 blocks
    # of K -- every test above -- or, with FEMSHELL_AMG_KEEP_HOST=1, up to 2,000,000; beyond that the solve does not pay for them
    m, mat = _make("panel", 224)  # 100,352 triangles, 50,625 nodes, 352,801 blocks
    for keep in (False, True):
        if keep:
            monkeypatch.setenv("FEMSHELL_AMG_KEEP_HOST", "1")
        fs = _context(m, mat)
        fs.set_preconditioner("amg")
        u, info = fs.solve(rtol=1e-8, max_it=500)
        assert info["converged"] == 1 and info["amg_levels"] >= 3
        ex = fs.amg_export(0)
        if keep:
            assert ex["P_vals"] is not None and len(ex["P_cols"]) == fs.amg_levels()[0]["p_blocks"]
            assert len(ex["A_cols"]) == fs.amg_levels()[0]["nnz_blocks"]
        else:
            assert ex["P_vals"] is None or len(ex["P_vals"]) == 0
        last = fs.amg_export(info["amg_levels"] - 1)  # the coarsest operator and its inverse: at every size
        assert last["A_vals"] is not None and len(last["A_vals"]) > 0 and last["coarse_inverse"] is not None
        fs.close()


def test_solve_seconds_is_the_krylov_loop_without_the_setup():
    # femshell_solve_info: pc_setup_seconds and solve_seconds are separate figures (bench.py's time to solution is the second);
    # the first solve of a context builds the hierarchy, the second reuses it, and both report the same loop time
    m, mat = _make("panel", 160)
    fs = _context(m, mat)
    fs.set_preconditioner("amg")
    u1, i1 = fs.solve(rtol=1e-10, max_it=500)
    u2, i2 = fs.solve(rtol=1e-10, max_it=500)
    assert i1["pc_setup_seconds"] > 0.0 and i2["pc_setup_seconds"] == 0.0
    assert i1["iterations"] == i2["iterations"]
    assert i1["solve_seconds"] < 1.3 * i2["solve_seconds"] + 0.005, (i1["solve_seconds"], i2["solve_seconds"], i1["pc_setup_seconds"])
    assert i1["pc_setup_seconds"] > 0.3 * i2["solve_seconds"]  # (a setup inside solve_seconds would have shown above)
    fs.close()


def test_very_thin_strip_keeps_its_coarsest_inverse_in_double_precision(monkeypatch):
    # a cantilever strip of t / L = 1 / 1600: the coarsest operator (485 nodes) is so ill-conditioned that its inverse rounded
    # to float is not positive definite any more -- the flexible CG broke down on it.  The setup measures what rounding did
    # (||A inv32 v - v|| / ||v||) and keeps the FP64 inverse; the solve converges to the direct solution without a fallback
    m = meshes.structured(256, 16, 0, 0, 16.0, 1.0, kind="t", ul_lr=True, bcids=(-1, -1, 1, -1), factor=300.0, loading=2)
    mat = (0.3, 1e7, 0.01)
    fs = _context(m, mat)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-10, max_it=1000)
    assert info["converged"] == 1 and info["amg_levels"] == 2 and info["pc_fp64_fallback"] == 0, info
    rg, cg, vg, Fg = fs.export_bsr()
    ug = oracle.refined_solve(rg, cg, vg, Fg)
    assert np.linalg.norm(u.ravel() - ug) / np.linalg.norm(ug) < 1e-8  # (kappa ~ 1e13: 1.3e-10 measured)
    fs.close()


def test_breakdown_under_single_precision_copies_runs_again_in_double_precision(monkeypatch):
    # an unstructured Delaunay shell of poor element quality (the mesh of tests/test_gpu_parity.py) WITHOUT the patch smoother of
    # round 6 (FEMSHELL_AMG_PATCH_TAU=0: with it the level keeps FP64 copies from the start and the solve converges, below): the
    # point-block multigrid does not converge on it in either precision, but with the single-precision copies the flexible CG breaks
    # down early (p.Ap <= 0).  femshell_solve then builds the hierarchy again, all FP64, runs the solve from the start and
    # says so; the context stays with that choice
    from tests.test_gpu_parity import delaunay_shell

    monkeypatch.setenv("FEMSHELL_AMG_PATCH_TAU", "0")
    ensure_built()
    xyz, tri = delaunay_shell(20000, 3)
    dmask = np.zeros(len(xyz), dtype=np.uint8)
    dmask[xyz[:, 0] < 0.15] = 0x3F
    loads = np.zeros((len(xyz), 6))
    loads[:, 2] = 1.0
    fs = pkg.FemShell(0.3, 7.0e4, 0.03, device=0)
    fs.set_mesh(xyz, tri, None)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-10, max_it=150)  # (no exception: the second attempt ends at the iteration limit)
    assert info["pc_fp64_fallback"] == 1 and info["converged"] == 0 and info["iterations"] == 150, info
    assert np.all(np.isfinite(u))
    u2, info2 = fs.solve(rtol=1e-10, max_it=150)  # the hierarchy is FP64 now: no second fallback, the same iterate
    assert info2["pc_fp64_fallback"] == 0 and info2["pc_setup_seconds"] == 0.0
    np.testing.assert_array_equal(u2, u)
    fs.close()


def test_tentative_prolongator_with_the_rows_in_memory(monkeypatch):
    # aggregates of more than 42 nodes keep the rows of their QR factorisation in HBM instead of registers; no test mesh
    # has one, so the knob sends every aggregate down that path
    monkeypatch.setenv("FEMSHELL_AMG_QR", "memory")
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    test_hierarchy_and_iteration_counts_follow_the_restatement("K")


def test_double_double_residual_and_what_refinement_buys():
    # thin roof: ||K|| ||x|| / ||b|| ~ 1e7.  The FP64 residual of a converged iterate is rounding noise, the
    # double-double one is exact to 1e-12 ||b||; without refinement the displacement error stalls near kappa*eps,
    # one pass takes it down by orders of magnitude
    m, mat = _make("roof", 96)
    fs = _context(m, mat)
    fs.set_preconditioner("amg", refine_passes=0)
    u0, i0 = fs.solve(rtol=1e-12, max_it=500)
    rg, cg, vg, Fg = fs.export_bsr()
    A = _bsr(rg, cg, vg, m.n_nodes)
    r_ext = amg_oracle.residual_extended(A, Fg, u0.ravel())
    r_dd = fs.residual(u0)
    r_f64 = Fg - A @ u0.ravel()
    nb = np.linalg.norm(Fg)
    assert np.linalg.norm(r_dd - r_ext) <= 1e-11 * nb
    assert np.linalg.norm(r_f64 - r_ext) >= 50 * np.linalg.norm(r_dd - r_ext)  # FP64 evaluation: noise
    assert abs(i0["true_rel_residual"] - np.linalg.norm(r_ext) / nb) <= 1e-3 * i0["true_rel_residual"]
    ug = oracle.refined_solve(rg, cg, vg, Fg)
    e0 = np.linalg.norm(u0.ravel() - ug) / np.linalg.norm(ug)
    fs.set_preconditioner("amg", refine_passes=1)
    u1, i1 = fs.solve(rtol=1e-12, max_it=500)
    e1 = np.linalg.norm(u1.ravel() - ug) / np.linalg.norm(ug)
    assert i1["iterations"] > i0["iterations"] and e1 < 1e-12 and e1 < 0.05 * e0, (e0, e1)
    fs.close()


def test_config1_scordelis_lo_250k_converged_against_the_direct_solve():
    """BASELINE.json configs[1] at full size: 354 x 354 squares = 250,632 tri3, 756,150 dofs, solved to rtol 1e-12.
    Solver term: against the oracle's refined direct solve of the matrix the GPU assembled, < 1e-10 (north star).
    Total: against the oracle's own assembly + direct solve; the two FP64 assemblies agree to 1e-14 and kappa carries
    that to ~2e-8 in the displacements -- any two correct FP64 implementations differ by that."""
    m, mat = _make("roof", 354)
    assert len(m.tri) == 250632
    fs = _context(m, mat)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=1000)
    assert info["converged"] == 1 and info["iterations"] < 400
    rg, cg, vg, Fg = fs.export_bsr()
    ug = oracle.refined_solve(rg, cg, vg, Fg, sweeps=4)
    solver_err = np.linalg.norm(u.ravel() - ug) / np.linalg.norm(ug)
    assert solver_err < 1e-10, solver_err
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, oracle.material(*mat), m.dirichlet_mask(), m.loads)
    assert np.abs(vg - v0).max() <= 1e-12 * np.abs(v0).max()
    assert np.array_equal(Fg, F0)
    u0 = oracle.refined_solve(r0, c0, v0, F0, sweeps=4)
    total = np.linalg.norm(u.ravel() - u0) / np.linalg.norm(u0)
    sensitivity = np.linalg.norm(ug - u0) / np.linalg.norm(u0)
    assert total < 1e-6 and abs(total - sensitivity) < 1e-10, (total, sensitivity)
    print("config1 250k roof: %d iterations, %.3f s, solver term %.2e, total %.2e (two assemblies: %.2e)"
          % (info["iterations"], info["solve_seconds"], solver_err, total, sensitivity))
    fs.close()


EXAMPLES = [("test_A_uv_t", 0.25, 30000.0, 1.0), ("test_B_uv_q", 0.25, 30000.0, 1.0), ("test_C_w_tA16", 0.3, 10.92, 1.0),
            ("test_D_w_q_uni16", 0.3, 1e7, 0.5), ("test_E_uvw_t", 0.25, 30000.0, 1.0), ("test_F_032_ss_uni", 0.3, 1.7472e7, 0.01),
            ("test_G_mpi_64_q", 0.3, 1e7, 0.5)]


@pytest.mark.parametrize("name,nu,E,t", EXAMPLES)
def test_solver_term_is_below_1e10_on_every_shipped_example(name, nu, E, t):
    """north star: displacements within 1e-10 of the reference path.  What a solver can be held to is the solver term --
    its result against the (refined) direct solve of the same matrix; the multigrid solve with one refinement pass meets
    1e-10 on every shipped example, the thin plate F (t = 0.01) and the 64 x 64 mesh G included, where block-Jacobi CG
    alone stalls at 1e-9 ... 1e-7.  The remainder of the total error is kappa times the 1e-15 rounding difference of
    two FP64 assemblies and belongs to the problem, not the solver."""
    m = meshes.load_example(name)
    fs = _context(m, (nu, E, t))
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-12, max_it=2000)
    assert info["converged"] == 1
    rg, cg, vg, Fg = fs.export_bsr()
    ug = oracle.refined_solve(rg, cg, vg, Fg)
    solver_term = np.linalg.norm(u.ravel() - ug) / np.linalg.norm(ug)
    assert solver_term < 1e-10, solver_term
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, oracle.material(nu, E, t), m.dirichlet_mask(), m.loads)
    assert np.abs(vg - v0).max() <= 1e-12 * np.abs(v0).max()
    u0 = oracle.refined_solve(r0, c0, v0, F0)
    total = np.linalg.norm(u.ravel() - u0) / np.linalg.norm(u0)
    sensitivity = np.linalg.norm(ug - u0) / np.linalg.norm(u0)
    assert abs(total - sensitivity) < 2e-10, (total, sensitivity)
    print("%s: %d iterations, solver term %.1e, total %.1e = kappa-sensitivity %.1e" % (name, info["iterations"], solver_term, total, sensitivity))
    fs.close()


def test_hierarchy_is_reused_until_the_matrix_changes():
    m, mat = _make("roof", 40)
    fs = _context(m, mat)
    fs.set_preconditioner("amg")
    u1, i1 = fs.solve(rtol=1e-10, max_it=300)
    assert i1["pc_setup_seconds"] > 0.0
    fs.set_loads(2.0 * m.loads)
    u2, i2 = fs.solve(rtol=1e-10, max_it=300)
    assert i2["pc_setup_seconds"] == 0.0 and i2["converged"] == 1
    assert np.linalg.norm(u2 - 2.0 * u1) <= 1e-8 * np.linalg.norm(u2)
    # a new Dirichlet set changes K: the hierarchy is rebuilt
    dm = m.dirichlet_mask()
    dm[m.n_nodes // 2] = 0x3F
    fs.set_dirichlet(dm)
    u3, i3 = fs.solve(rtol=1e-10, max_it=300)
    assert i3["pc_setup_seconds"] > 0.0 and i3["converged"] == 1
    assert np.abs(u3[m.n_nodes // 2]).max() == 0.0
    # bitwise reproducible
    u4, i4 = fs.solve(rtol=1e-10, max_it=300)
    assert np.array_equal(u3, u4) and i3["iterations"] == i4["iterations"]
    fs.close()


def test_restriction_rows_wider_than_the_lds_panel(monkeypatch):
    """On this Delaunay mesh (slivers on the hull, Morton numbering) a coarse node of level 1 collects from 162 fine
    nodes: k_spmv stages the x entries of at most 64 block columns in LDS at a time and goes through wider slices in
    several passes (the launch used to fail with 'invalid argument' beyond 106 columns = 160 KiB).  (The point-block
    hierarchy of rounds 2-5: with the patch smoother this mesh has two levels and no such row.)"""
    from tests.test_gpu_parity import delaunay_shell
    monkeypatch.setenv("FEMSHELL_AMG_PATCH_TAU", "0")
    xyz, tri = delaunay_shell(2500, 5)
    n = len(xyz)
    rng = np.random.default_rng(3)
    fs = pkg.FemShell(0.3, 7.0e4, 0.03, flags=pkg.REF_DEFAULT | pkg.REORDER_MORTON)
    fs.set_mesh(xyz, tri)
    fixed = np.flatnonzero(xyz[:, 0] < 0.2).astype(np.int32)
    fs.set_dirichlet(np.full(len(fixed), 0x3F, np.uint8), node_ids=fixed)
    fs.set_loads(rng.normal(size=(n, 6)))
    fs.set_preconditioner("amg", coarsest_nodes=200)  # (three levels: the wide restriction is the one onto the coarsest)
    u, info = fs.solve(rtol=1e-8, max_it=4000)
    assert info["converged"] == 1 and info["amg_levels"] >= 3
    lv = fs.amg_levels()
    assert lv[1]["n_nodes"] < 400
    r, c, v, F = fs.export_bsr()
    u_ref = oracle.refined_solve(r, c, v, F)
    assert np.linalg.norm(u.ravel() - u_ref) <= 1e-4 * np.linalg.norm(u_ref)  # kappa ~ 1e13 on this mesh


def test_multigrid_through_a_one_rank_rccl_communicator(monkeypatch):
    # the row-partitioned multigrid path (csrc/amg_dist.cpp: rank-local aggregation, row exchanges of the setup, halo products
    # and all-reduced K-cycle sums in the cycle) with the real librccl, on the one GPU a test box has: one rank's aggregates
    # are the single-rank ones, so same iterations and solution as without a communicator
    m = meshes.structured(40, 36, 0, 0, 10, 9, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
    m.xyz[:, 2] = 0.4 * np.sin(0.5 * m.xyz[:, 0]) * np.cos(0.4 * m.xyz[:, 1])
    ref = pkg.FemShell(0.3, 1e7, 0.1)
    ref.set_mesh(m.xyz, m.tri)
    ref.set_dirichlet(m.dirichlet_mask())
    ref.set_loads(m.loads)
    ref.set_preconditioner("amg", coarsest_nodes=60)
    u0, i0 = ref.solve(rtol=1e-11, max_it=2000)
    monkeypatch.setenv("FEMSHELL_FORCE_COMM", "1")
    fs = pkg.FemShell(0.3, 1e7, 0.1, rank=0, world_size=1)
    fs.comm_init(pkg.comm_unique_id())
    monkeypatch.delenv("FEMSHELL_FORCE_COMM")
    fs.set_mesh(m.xyz, m.tri)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    fs.set_preconditioner("amg", coarsest_nodes=60)
    u1, i1 = fs.solve(rtol=1e-11, max_it=2000)
    assert i0["converged"] == 1 and i1["converged"] == 1 and i1["amg_levels"] == i0["amg_levels"] >= 2
    assert abs(i1["iterations"] - i0["iterations"]) <= 2
    assert np.linalg.norm(u1 - u0) <= 1e-10 * np.linalg.norm(u0)
    u2, i2 = fs.solve(rtol=1e-11, max_it=2000)  # hierarchy reused
    assert i2["pc_setup_seconds"] == 0.0 and np.array_equal(u2, u1)
    # K changes (another Dirichlet set): the hierarchy is built again
    dm2 = m.dirichlet_mask().copy()
    dm2[m.n_nodes // 2] |= 0x3F
    for ctx in (fs, ref):
        ctx.set_dirichlet(dm2)
    u3, i3 = fs.solve(rtol=1e-11, max_it=2000)
    u3r, i3r = ref.solve(rtol=1e-11, max_it=2000)
    assert i3["converged"] == 1 and i3["pc_setup_seconds"] > 0.0 and abs(i3["iterations"] - i3r["iterations"]) <= 2
    assert np.linalg.norm(u3 - u3r) <= 1e-10 * np.linalg.norm(u3r) and np.linalg.norm(u3 - u1) > 1e-6 * np.linalg.norm(u1)


def test_flap_loaded_in_its_plane_converges_like_the_plates():
    # the coupled example's structure: a 0.1 x 1 flap in the x-z plane, bottom edge clamped, forces along x (in its plane).
    # The soft modes there are rigid rotations with NO nodal rotation about the normal (the drilling stiffness is an
    # uncoupled penalty): with the plain rigid-body modes as near-null space this took 715 iterations at this size
    nx, nz = 50, 100
    m = meshes.structured(nx, nz, 0, 0, 0.1, 1.0, kind="t", ul_lr=True, bcids=(2, 20, 2, 2), factor=1.0, loading=0, dead_axis="y")
    loads = np.zeros((m.n_nodes, 6))
    loads[np.abs(m.xyz[:, 0]) < 1e-12, 0] = 1.0
    fs = pkg.FemShell(0.3, 1e6, 0.1)
    fs.set_mesh(m.xyz, m.tri)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(loads)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-11, max_it=2000)
    assert info["converged"] == 1 and info["amg_levels"] >= 2
    assert info["iterations"] < 120, info["iterations"]
    mat = oracle.material(0.3, 1e6, 0.1)
    r0, c0, v0, F0 = oracle.assemble(m.xyz, m.tri, m.quad, mat, m.dirichlet_mask(), loads)
    rg, cg, vg, Fg = fs.export_bsr()
    ud = oracle.refined_solve(rg, cg, vg, Fg)
    assert np.linalg.norm(u.ravel() - ud) <= 1e-10 * np.linalg.norm(ud)
    # the numpy restatement builds the same near-null space (tangent-plane projection with the node normals)
    N = amg_oracle.node_normals(m.xyz, m.tri)
    assert np.allclose(np.abs(N[:, 1]), 1.0) and np.allclose(N[:, [0, 2]], 0.0)
    B = amg_oracle.rigid_body_modes(m.xyz, None, N)
    assert np.allclose(B[:, 4, 4], 0.0) and np.allclose(B[:, 3, 3], 1.0) and np.allclose(B[:, 5, 5], 1.0)


@pytest.mark.parametrize("case", ["inplane", "folded", "strip"])
def test_multigrid_on_other_load_cases_and_shapes(case):
    # beyond the bending-dominated BASELINE configs (tools/amg_robustness_probe.py): a panel loaded in its plane, a plate
    # folded by 90 degrees (the drilling rotation of one half is a bending rotation of the other), a thin cantilever strip
    if case == "strip":
        m = meshes.structured(128, 8, 0, 0, 16.0, 1.0, kind="t", ul_lr=True, bcids=(-1, -1, 1, -1), factor=300.0, loading=2)
        mat, bound = (0.3, 1e7, 0.01), 150
        xyz, loads = m.xyz, m.loads
    else:
        m = meshes.structured(64, 64, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0) if case == "inplane" else (-1, -1, 1, -1),
                              factor=300.0, loading=2)
        mat, bound = (0.3, 1e7, 0.5), 120
        xyz, loads = m.xyz.copy(), np.zeros_like(m.loads)
        if case == "inplane":
            loads[:, 0] = 1.0
        else:
            right = m.xyz[:, 0] > 5.0
            xyz[right, 0] = 5.0
            xyz[right, 2] = m.xyz[right, 0] - 5.0
            loads[:, 2] = 1.0
    fs = pkg.FemShell(*mat)
    fs.set_mesh(xyz, m.tri)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(loads)
    fs.set_preconditioner("amg", coarsest_nodes=100)
    u, info = fs.solve(rtol=1e-11, max_it=1000)
    assert info["converged"] == 1 and info["amg_levels"] >= 2 and info["iterations"] < bound, info["iterations"]
    rg, cg, vg, Fg = fs.export_bsr()
    ud = oracle.refined_solve(rg, cg, vg, Fg)
    assert np.linalg.norm(u.ravel() - ud) <= 2e-10 * np.linalg.norm(ud)


@pytest.mark.parametrize("f32", [0, 1])
def test_dense_inverse_on_the_matrix_cores_equals_the_host_inverse(monkeypatch, f32):
    """csrc/amg_dense.hip: coarsest operators beyond 250 nodes are inverted by symmetric block sweeps on
    v_mfma_f64_16x16x4_f64.  Forced down to a 267-node coarsest level here (1602 dofs, 26 tiles) and held to the host's
    Cholesky inverse of the same operator: same iteration count, same solution; with the inverse stored in single
    precision (FEMSHELL_AMG_DENSE_F32=1) the preconditioner changes in the 8th digit and the iteration count by a step."""
    m, mat = _make("panel", 48)
    out = {}
    for path, dmin in (("host", "100000"), ("device", "0"), ("device128", "0")):
        monkeypatch.setenv("FEMSHELL_AMG_DENSE_DEVICE_MIN", dmin)
        monkeypatch.setenv("FEMSHELL_AMG_DENSE_F32", str(f32))
        # (device128: the trailing update on 128 x 128 tiles, the measured alternative of round 5 -- same inverse)
        monkeypatch.setenv("FEMSHELL_AMG_DENSE_TILE", "128" if path == "device128" else "64")
        fs = _context(m, mat)
        fs.set_preconditioner("amg", coarsest_nodes=300)
        u, info = fs.solve(rtol=1e-12, max_it=500)
        lv = fs.amg_levels()
        st = fs.amg_dense_stats()
        assert info["converged"] == 1 and len(lv) == 2 and 200 < lv[-1]["n_nodes"] <= 300
        out[path] = (u, info["iterations"], st, lv[-1]["n_nodes"])
        if path.startswith("device"):
            # the inverse the matrix cores computed against the CHECKER's coarsest operator (oracle/amg_oracle.py builds its own
            # hierarchy from the exported K), not only against the product's host inverse
            rg, cg, vg, Fg = fs.export_bsr()
            levels = amg_oracle.setup(_bsr(rg, cg, vg, m.n_nodes), m.xyz, m.dirichlet_mask(), lams=[l["lambda_max"] for l in lv],
                                      coarsest_nodes=300, tri=m.tri, quad=m.quad)
            inv = fs.amg_export(len(lv) - 1)["coarse_inverse"]
            Ac = levels[-1].A.toarray()
            assert len(levels) == 2 and inv.shape == Ac.shape == (6 * lv[-1]["n_nodes"],) * 2
            defect = np.abs(Ac @ inv - np.eye(len(Ac))).max()
            assert defect <= (1e-9 if not f32 else 2e-4), defect
            # ... and, scaled to the operator, against LAPACK's inverse of the operator the library itself exports (nt = 26: two
            # super-blocks per XCD; the long-double truth of tests/test_gpu_dense_inverse.py stops at 1026 dofs): the distance of
            # two double methods is at most the sum of their errors, the device's is held to 4 x the restatement's, and a stored
            # float is rounded once more
            from tests.helpers import dense_truth

            ex = fs.amg_export(len(lv) - 1)
            Ae = _bsr(ex["A_rowptr"], ex["A_cols"], ex["A_vals"], lv[-1]["n_nodes"]).toarray()
            Ae = np.tril(Ae) + np.tril(Ae, -1).T  # (the device reads the lower triangle)
            lap = np.linalg.inv(Ae)
            restated, dropped, failed = dense_truth.restated_inverse(Ae)
            assert failed is None and dropped == []
            scale = np.abs(lap).max()
            allowed = dense_truth.bound(np.abs(restated - lap).max() / scale, len(Ae)) + (2.0 ** -24 if f32 else 0.0)
            dist = np.abs(inv - lap).max() / scale
            print("%s f32=%d: |device - lapack| / max|lapack| = %.2e, |restated - lapack| = %.2e, allowed %.2e"
                  % (path, f32, dist, np.abs(restated - lap).max() / scale, allowed))
            assert dist <= allowed, (dist, allowed)
        fs.close()
    assert out["device128"][1] == out["device"][1] and np.linalg.norm(out["device128"][0] - out["device"][0]) <= 1e-12 * np.linalg.norm(out["device"][0])
    assert out["host"][2]["n"] == 0 and out["device"][2]["n"] == 6 * out["device"][3]
    assert out["device"][2]["dropped_directions"] == 0 and out["device"][2]["mfma_flops_issued"] > 0
    assert abs(out["host"][1] - out["device"][1]) <= (2 if f32 else 1), (out["host"][1], out["device"][1])
    assert np.linalg.norm(out["host"][0] - out["device"][0]) <= 1e-10 * np.linalg.norm(out["host"][0])


def test_dense_inverse_runs_again_without_the_look_ahead_when_its_wait_expires(monkeypatch):
    """The look-ahead's pivot launch (second stream) waits, bounded, for three workgroups of the update on the first stream, and
    the next panel kernel for the pivot launch (csrc/amg_dense.hip).  If the two streams do not run side by side, or on a card
    shared with other processes, a wait can expire: the setup then runs the inverse again with the pivot as a launch in front of
    every sweep instead of failing.  Forced here by a spin limit of zero; same solution as with the look-ahead."""
    m, mat = _make("panel", 48)
    sols = {}
    for spins in (None, "0"):
        monkeypatch.setenv("FEMSHELL_AMG_DENSE_DEVICE_MIN", "0")
        if spins is None:
            monkeypatch.delenv("FEMSHELL_AMG_DENSE_LOOKAHEAD_SPINS", raising=False)
        else:
            monkeypatch.setenv("FEMSHELL_AMG_DENSE_LOOKAHEAD_SPINS", spins)
        fs = _context(m, mat)
        fs.set_preconditioner("amg", coarsest_nodes=300)
        u, info = fs.solve(rtol=1e-12, max_it=500)
        assert info["converged"] == 1 and fs.amg_dense_stats()["n"] > 1200
        sols[spins] = (u, info["iterations"])
        fs.close()
    assert sols[None][1] == sols["0"][1]
    np.testing.assert_array_equal(sols[None][0], sols["0"][0])


def test_dense_inverse_look_ahead_in_a_process_with_many_streams(monkeypatch):
    """The look-ahead of the dense inverse runs on a second stream of the context and meets the first through device-side counters
    (csrc/amg_dense.hip).  HIP maps streams onto a few hardware queues: in a process with many contexts the two streams of one
    can share a queue, and the pivot launch would wait -- for its full bound -- for an update queued BEHIND it.  The context
    asks once whether its streams run side by side and does without the look-ahead if not: setups stay in the tens of
    milliseconds whatever the answer is, and the solution is the same."""
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_DEVICE_MIN", "0")
    m, mat = _make("panel", 48)
    keep, times, sols = [], [], []
    for k in range(7):  # fourteen streams in the end
        fs = _context(m, mat)
        fs.set_preconditioner("amg", coarsest_nodes=300)
        u, info = fs.solve(rtol=1e-12, max_it=500)
        assert info["converged"] == 1 and fs.amg_dense_stats()["n"] > 1200
        times.append(info["pc_setup_seconds"])
        sols.append((u, info["iterations"]))
        keep.append(fs)
    for fs in keep:
        fs.close()
    assert max(times[1:]) < 0.25, times  # (a bound that expired cost more than a second; the first setup loads the code objects)
    for u, its in sols[1:]:
        assert abs(its - sols[0][1]) <= 1
        assert np.linalg.norm(u - sols[0][0]) <= 1e-9 * np.linalg.norm(sols[0][0])


def test_dense_inverse_on_the_matrix_cores_drops_semi_definite_directions(monkeypatch):
    """The reference's Test A fixes u, v, w at three collinear nodes only: the rotation about that line has no stiffness,
    and the inverse of the coarsest operator (here K itself, 27 nodes) has to drop it -- same rule on the device as on the
    host (pivot that lost eleven digits against its diagonal entry), same displacements."""
    m = meshes.load_example("test_A_uv_t")
    sols = {}
    for path, dmin in (("host", "100000"), ("device", "0")):
        monkeypatch.setenv("FEMSHELL_AMG_DENSE_DEVICE_MIN", dmin)
        fs = _context(m, (0.25, 30000.0, 1.0))
        fs.set_preconditioner("amg")
        u, info = fs.solve(rtol=1e-12, max_it=200)
        assert info["converged"] == 1
        sols[path] = (u, fs.amg_dense_stats())
        fs.close()
    assert sols["device"][1]["n"] == 6 * m.n_nodes and sols["device"][1]["dropped_directions"] >= 1
    rg = np.linalg.norm(sols["host"][0] - sols["device"][0]) / np.linalg.norm(sols["host"][0])
    assert rg < 1e-9, rg


@pytest.mark.parametrize("flag", ["REORDER_MORTON", "REORDER_RCM"])
def test_aggregates_do_not_depend_on_the_internal_numbering(flag):
    """With FEMSHELL_REORDER_* the library numbers the nodes its own way (csrc/reorder.cpp), and the greedy aggregation
    passes depend on the order in which they meet the nodes.  They follow the caller's numbering in that case (visiting
    order and the tie-break of the leftovers: csrc/amg_setup.cpp aggregate_nodes), so the hierarchy -- level sizes and
    iteration count -- is the one of the context without the flag (the 4M-triangle cylinder went from 139 to 443
    iterations under Morton numbering before)."""
    m, mat = _make("cylinder", 160)
    out = {}
    for name, flags in (("plain", pkg.REF_DEFAULT), ("reordered", pkg.REF_DEFAULT | getattr(pkg, flag))):
        ensure_built()
        fs = pkg.FemShell(*mat, device=0, flags=flags)
        fs.set_mesh(m.xyz, m.tri, m.quad)
        fs.set_dirichlet(m.dirichlet_mask())
        fs.set_loads(m.loads)
        fs.set_preconditioner("amg", coarsest_nodes=200)
        u, info = fs.solve(rtol=1e-10, max_it=2000)
        assert info["converged"] == 1
        out[name] = (u, info["iterations"], [lv["n_nodes"] for lv in fs.amg_levels()])
        fs.close()
    assert out["reordered"][2] == out["plain"][2], (out["plain"][2], out["reordered"][2])
    assert abs(out["reordered"][1] - out["plain"][1]) <= 0.1 * out["plain"][1] + 2, (out["plain"][1], out["reordered"][1])
    assert np.linalg.norm(out["reordered"][0] - out["plain"][0]) <= 1e-7 * np.linalg.norm(out["plain"][0])


@pytest.mark.parametrize("pc", ["amg", "jacobi"])
def test_solve_from_an_initial_guess(pc):
    """femshell_set_initial_guess: what libMesh does for the reference -- system.solution goes to KSPSolve as the initial guess, so
    the solves of the coupled adapter's loop (fem-shell_precice.cpp:271) start from the last coupling iteration's displacements.
    From the previous solution and unchanged loads a solve needs a fraction of the iterations and returns the same displacements;
    from a scaled copy (the dummy fluid's load factor moving between time steps) it saves the decades the guess is worth; the
    guess is consumed by one solve; the multigrid path follows the restatement (oracle/amg_oracle.py solve x0)."""
    m, mat = _make("panel", 40)
    fs = _context(m, mat)
    if pc == "amg":
        fs.set_preconditioner("amg", coarsest_nodes=60)
    # (block-Jacobi CG in plain FP64: the explicit residual of a converged iterate sits at kappa x eps = 1e-9 ||b|| on this panel,
    #  whatever the recurrence reached -- a guess is worth something down to there, hence the tolerance of that leg)
    rtol = 1e-10 if pc == "amg" else 1e-8
    u_cold, cold = fs.solve(rtol=rtol, max_it=20000)
    assert cold["converged"] == 1
    # (1) from the previous solution where it lies
    fs.set_initial_guess(None)
    u1, i1 = fs.solve(rtol=rtol, max_it=20000)
    assert i1["converged"] == 1 and i1["iterations"] <= 0.45 * cold["iterations"], (i1["iterations"], cold["iterations"])
    assert np.linalg.norm(u1 - u_cold) <= (1e-9 if pc == "amg" else 1e-6) * np.linalg.norm(u_cold)
    # (2) consumed: the next solve starts from zero again
    u2, i2 = fs.solve(rtol=rtol, max_it=20000)
    assert i2["iterations"] == cold["iterations"]
    np.testing.assert_array_equal(u2, u_cold)
    # (3) loads scaled by 1.04, guess = the old solution handed in from the host: the answer is 1.04 x, in fewer iterations
    fs.set_loads(1.04 * m.loads)
    fs.set_initial_guess(u_cold)
    u3, i3 = fs.solve(rtol=rtol, max_it=20000)
    assert i3["converged"] == 1 and i3["iterations"] < cold["iterations"]
    assert np.linalg.norm(u3 - 1.04 * u_cold) <= (1e-8 if pc == "amg" else 1e-5) * np.linalg.norm(u_cold)
    if pc == "amg":
        lv = fs.amg_levels()
        rg, cg, vg, Fg = fs.export_bsr()
        A = _bsr(rg, cg, vg, m.n_nodes)
        levels = amg_oracle.setup(A, m.xyz, m.dirichlet_mask(), lams=[l["lambda_max"] for l in lv], coarsest_nodes=60, tri=m.tri, quad=m.quad)
        u0, hist = amg_oracle.solve(A, Fg, levels, rtol=rtol, max_it=400, refine_passes=1, x0=u_cold.ravel())
        assert abs(len(hist) - i3["iterations"]) <= 2, (len(hist), i3["iterations"])
        assert np.linalg.norm(u3.ravel() - u0) <= 1e-9 * np.linalg.norm(u0)
    # (4) errors: before any solve of a fresh context there is nothing to start from
    fs2 = _context(m, mat)
    with pytest.raises(pkg.FemShellError):
        fs2.set_initial_guess(None)
    fs2.close()
    fs.close()


def _poor_shell(n_pts, seed, along_x=False):
    from tests.test_gpu_parity import delaunay_shell

    xyz, tri = delaunay_shell(n_pts, seed)
    if along_x:  # numbered along x, as tests/helpers/multirank_worker.py numbers the same shell for several ranks
        order = np.argsort(xyz[:, 0], kind="stable")
        inv = np.empty_like(order)
        inv[order] = np.arange(len(order))
        xyz, tri = np.ascontiguousarray(xyz[order]), inv[tri].astype(np.int32)
    n = len(xyz)
    dmask = np.zeros(n, dtype=np.uint8)
    dmask[xyz[:, 0] < 0.15] = 0x3F
    loads = np.zeros((n, 6))
    loads[:, 2] = 1.0
    return xyz, tri, dmask, loads


def test_patch_smoother_on_a_shell_of_poor_element_quality_follows_the_restatement(monkeypatch):
    """Round 6, csrc/amg_patch.hpp: a 3000-point random Delaunay shell -- nodes a hundredth of the mesh width
    apart -- on which the point-block multigrid does not converge.  The clusters the device finds equal the restatement's, the
    hierarchy (glued aggregates, P smoothed with the cluster blocks, Galerkin operator, spectral bound) equals the restatement's
    level by level, the solve converges in about the restatement's iterations, without the FP64 rebuild, to the direct solve's answer;
    switched off (FEMSHELL_AMG_PATCH_TAU=0) the same solve does not converge in twice as many iterations."""
    ensure_built()
    xyz, tri, dmask, loads = _poor_shell(3000, 2)
    n = len(xyz)
    fs = pkg.FemShell(0.3, 7.0e4, 0.03, device=0)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-10, max_it=600)
    assert info["converged"] == 1 and info["pc_fp64_fallback"] == 0 and info["iterations"] <= 400, info
    pi = fs.amg_patch_info()
    assert pi["clusters"] > 500 and pi["nodes_in_clusters"] > 1500 and pi["not_positive_definite"] == 0 and pi["max_nodes"] == 8
    lv = fs.amg_levels()
    rg, cg, vg, Fg = fs.export_bsr()
    A = _bsr(rg, cg, vg, n)
    ex = fs.amg_export(0)
    labels = ex["patch_labels"]
    Dinv = amg_oracle.block_diag_inverse(A)
    ea, ec, s2 = amg_oracle.patch_edges(A, Dinv, 0.8)
    lab_o, ptr_o, nodes_o = amg_oracle.patch_clusters(n, ea, ec, s2, 8)
    # (an edge whose sigma sits within rounding of tau may fall on either side -- the device contracts its products into FMAs --: the
    #  two edge sets agree up to a handful of edges and the partitions up to the clusters those touch; the hierarchy below is restated
    #  from the library's own labels)
    assert abs(pi["rigid_edges"] - len(ea)) <= 3, (pi["rigid_edges"], len(ea))
    members = lambda lab: [frozenset(np.flatnonzero(lab == lab[i]).tolist()) if lab[i] >= 0 else frozenset([i]) for i in range(n)]  # noqa: E731
    differing = sum(a != b for a, b in zip(members(labels), members(lab_o)))
    assert differing <= 24, differing
    sizes = np.bincount(labels[labels >= 0])
    assert sizes.min() >= 2 and sizes.max() <= 8
    levels = amg_oracle.setup(A, xyz, dmask, lams=[l["lambda_max"] for l in lv], coarsest_nodes=1400, tri=tri, patch_labels=labels)
    assert [L.n for L in levels] == [l["n_nodes"] for l in lv]
    np.testing.assert_array_equal(ex["agg"], levels[0].agg)
    P = _bsr(ex["P_rowptr"], ex["P_cols"], ex["P_vals"], lv[0]["n_coarse"])
    # (the inverses of cluster blocks whose nodes nearly coincide -- condition numbers of 1e8 and beyond -- come out of two different
    #  factorisations: P agrees to the digits those leave, where it agrees to 1e-11 on meshes without clusters)
    assert abs(P - levels[0].P).max() <= 2e-6 * abs(levels[0].P).max()
    ex1 = fs.amg_export(1)
    A1 = _bsr(ex1["A_rowptr"], ex1["A_cols"], ex1["A_vals"], lv[1]["n_nodes"])
    assert abs(A1 - levels[1].A).max() <= 1e-5 * abs(levels[1].A).max()
    assert 0.9 * lv[0]["lambda_max"] <= 1.1 * amg_oracle.lambda_max(levels[0].A, levels[0].Dm, 60) <= 1.25 * lv[0]["lambda_max"]
    u0, hist = amg_oracle.solve(A, Fg, levels, rtol=1e-10, max_it=600, refine_passes=1)
    assert abs(len(hist) - info["iterations"]) <= 0.1 * len(hist) + 5, (len(hist), info["iterations"])
    # (slivers make these systems so ill-conditioned that the refined direct solve itself is good to 1e-7 or so:
    #  tests/test_gpu_parity.py test_unstructured_delaunay_shell holds its 700-point sibling to 1e-5)
    ug = oracle.refined_solve(rg, cg, vg, Fg)
    assert np.linalg.norm(u.ravel() - ug) / np.linalg.norm(ug) < 1e-6
    assert np.linalg.norm(u.ravel() - u0) / np.linalg.norm(u0) < 1e-6
    fs.close()
    monkeypatch.setenv("FEMSHELL_AMG_PATCH_TAU", "0")
    fs = pkg.FemShell(0.3, 7.0e4, 0.03, device=0)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.set_preconditioner("amg")
    _, info0 = fs.solve(rtol=1e-10, max_it=2 * info["iterations"])
    assert info0["converged"] == 0 and fs.amg_patch_info()["clusters"] == 0
    fs.close()


def test_patch_smoother_takes_the_20k_point_shell_below_400_iterations():
    """The shell of tests/test_multirank_gpu.py (20,000 random points, numbered along x): > 1000 iterations with point blocks in
    rounds 3-5; with the cluster blocks <= 400, no FP64 rebuild, answer equal to the refined direct solve's."""
    ensure_built()
    xyz, tri, dmask, loads = _poor_shell(20000, 3, along_x=True)
    fs = pkg.FemShell(0.3, 7.0e4, 0.03, device=0)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.set_preconditioner("amg")
    u, info = fs.solve(rtol=1e-10, max_it=600)
    assert info["converged"] == 1 and info["pc_fp64_fallback"] == 0 and info["iterations"] <= 400, info
    rg, cg, vg, Fg = fs.export_bsr()
    ug = oracle.refined_solve(rg, cg, vg, Fg)
    assert np.linalg.norm(u.ravel() - ug) / np.linalg.norm(ug) < 1e-5
    fs.close()


def test_structured_meshes_have_no_clusters_and_keep_their_bits(monkeypatch):
    """No rigid edge on a mesh of decent element quality: nothing of the patch smoother runs, hierarchy and iterates are the ones of
    FEMSHELL_AMG_PATCH_TAU=0 bit for bit."""
    m, mat = _make("cylinder", 48)
    out = []
    for tau in (None, "0"):
        if tau is not None:
            monkeypatch.setenv("FEMSHELL_AMG_PATCH_TAU", tau)
        fs = _context(m, mat)
        fs.set_preconditioner("amg", coarsest_nodes=60)
        u, info = fs.solve(rtol=1e-10, max_it=400)
        assert fs.amg_patch_info()["rigid_edges"] == 0 and fs.amg_export(0)["patch_labels"] is None
        out.append((u.copy(), info["iterations"], fs.residual_history().copy()))
        fs.close()
    assert out[0][1] == out[1][1]
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][2], out[1][2])


def _delaunay_context(n_pts, seed):
    ensure_built()
    xyz, tri = meshes.delaunay_patch(n_pts, seed)
    n = len(xyz)
    dmask = np.zeros(n, dtype=np.uint8)
    dmask[xyz[:, 0] < 0.1] = 0x3F
    loads = np.zeros((n, 6))
    loads[:, 2] = 1.0
    fs = pkg.FemShell(0.3, 1e7, 0.05, device=0)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    return fs


@pytest.mark.parametrize("kind,n,coarse_sym", [("panel", 64, "100000"), ("panel", 64, "1"), ("quads", 40, "1"), ("cylinder", 48, "100000"),
                                               ("delaunay", 6000, "1"), ("delaunay", 6000, "100000"), ("full", 56, "1"), ("mixed", 40, "1")])
def test_patterns_built_in_hbm_are_the_hosts_lists_slot_for_slot(monkeypatch, kind, n, coarse_sym):
    """Round 6, csrc/amg_symbolic.hip: the patterns of P, A P, R, A_c, the maps from the blocks of A to the slots
    of P and the in-lists of a symmetric A_c are built in HBM, one lane per row; the greedy passes of the aggregation run on the
    operator's ELL pattern without the sorted graph.  FEMSHELL_AMG_SYMBOLIC=host keeps the host's lists of rounds 3-5.  Same
    aggregates, same operators, same iterates -- bit for bit, on every level coarsened on the device (forced down to 100-node
    levels), with full and with symmetric storage of the coarse operators, on structured and on Delaunay meshes."""
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    monkeypatch.setenv("FEMSHELL_AMG_COARSE_SYM", coarse_sym)
    if kind == "full":  # K itself stored in full (no in-lists on level 0), the coarse operators symmetric
        monkeypatch.setenv("FEMSHELL_SYMMETRIC", "0")
    out = []
    for where in ("device", "host"):
        monkeypatch.setenv("FEMSHELL_AMG_SYMBOLIC", where)
        if kind == "delaunay":
            fs = _delaunay_context(n, 5)
        elif kind == "mixed":  # triangles and quadrilaterals in one mesh
            m, mat = _make("quads", n)
            half = len(m.quad) // 2
            tri = np.concatenate([m.quad[half:, [0, 1, 2]], m.quad[half:, [0, 2, 3]]]).astype(np.int32)
            ensure_built()
            fs = pkg.FemShell(*mat, device=0)
            fs.set_mesh(m.xyz, tri, m.quad[:half])
            fs.set_dirichlet(m.dirichlet_mask())
            fs.set_loads(m.loads)
        else:
            fs = _context(*_make("panel" if kind == "full" else kind, n))
        fs.set_preconditioner("amg", coarsest_nodes=60)
        u, info = fs.solve(rtol=1e-10, max_it=600)
        assert info["converged"] == 1, info
        lv = fs.amg_levels()
        assert len(lv) >= 3
        ex = [fs.amg_export(li) for li in range(len(lv) - 1)]
        st = fs.amg_setup_stats()
        out.append((u.copy(), info["iterations"], fs.residual_history().copy(), lv, ex, st))
        fs.close()
    dev, host = out
    assert dev[3] == host[3]
    assert dev[5]["galerkin_useful_flops"] == host[5]["galerkin_useful_flops"] > 0
    for a, b in zip(dev[4], host[4]):
        for key in ("agg", "A_rowptr", "A_cols", "A_vals", "P_rowptr", "P_cols", "P_vals"):
            assert (a[key] is None) == (b[key] is None), key
            if a[key] is not None:
                np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert dev[1] == host[1]
    np.testing.assert_array_equal(dev[2], host[2])
    np.testing.assert_array_equal(dev[0], host[0])


def _fan_mesh(valence, rings=6):
    """A dished disc of `rings` rings of `valence` nodes around a hub that is numbered LAST: the greedy passes reach the hub when its
    neighbours are taken, so its row of P sees every aggregate of the first ring."""
    pts = []
    for r in range(1, rings + 1):
        for k in range(valence):
            a = 2 * np.pi * (k + 0.5 * (r % 2)) / valence
            pts.append((r * np.cos(a), r * np.sin(a), 0.05 * r * r))
    hub = len(pts)
    pts.append((0.0, 0.0, 0.0))

    def idx(r, k):
        return (r - 1) * valence + (k % valence)

    tri = [(hub, idx(1, k), idx(1, k + 1)) for k in range(valence)]
    for r in range(1, rings):
        for k in range(valence):
            a, b, c, d = idx(r, k), idx(r, k + 1), idx(r + 1, k), idx(r + 1, k + 1)
            tri += [(a, c, d), (a, d, b)] if r % 2 else [(a, c, b), (b, c, d)]
    return np.array(pts), np.array(tri, dtype=np.int32)


def test_rows_beyond_the_lane_sets_take_the_hosts_lists(monkeypatch):
    """csrc/amg_symbolic.hip builds a row of P as a set of at most 64 aggregates in LDS (A P: 128, R and A_c: 256).  A hub of valence
    200 sees more (tools/lab/fan_probe.py: 67 and more from valence 200 on; beyond 240 an aggregate is seen by more than the 255 rows
    either path allows): the step says so (femshell_amg_symbolic_info), takes the host's lists and the solve goes on as if nothing had
    happened -- slowly: the triangles at the hub are needles of 1.8 degrees --; the level below is built in HBM again."""
    monkeypatch.setenv("FEMSHELL_AMG_PATCH_TAU", "0")  # (needle-shaped triangles at the hub: no cluster blocks, this test is about the lists)
    monkeypatch.setenv("FEMSHELL_AMG_DEVICE_MIN", "100")
    ensure_built()
    xyz, tri = _fan_mesh(200)
    n = len(xyz)
    dmask = np.zeros(n, dtype=np.uint8)
    dmask[np.hypot(xyz[:, 0], xyz[:, 1]) > 5.5] = 0x3F
    loads = np.zeros((n, 6))
    loads[:, 2] = 1.0
    fs = pkg.FemShell(0.3, 1e7, 0.2, device=0)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.set_preconditioner("amg", coarsest_nodes=60)
    u, info = fs.solve(rtol=1e-10, max_it=5000)
    where = fs.amg_symbolic_info()
    assert where["host_after_overflow"] >= 1 and where["in_hbm"] >= 1, where
    assert info["converged"] == 1, info
    rg, cg, vg, Fg = fs.export_bsr()
    ug = oracle.refined_solve(rg, cg, vg, Fg)
    assert np.linalg.norm(u.ravel() - ug) / np.linalg.norm(ug) < 1e-7
    fs.close()


def test_results_do_not_depend_on_what_recycled_device_memory_holds(tmp_path):
    """The device pool hands out used blocks (csrc/context.hpp DevPool: kept blocks, arenas, and since round 6 pieces carved from
    large kept blocks) where a fresh request to the driver would have been zero-filled.  FEMSHELL_POOL_POISON=1 fills every block
    with 0xFF bytes (NaN as a number, -1 as an index) before it is handed out: a child process solves the same systems that way --
    block-Jacobi and multigrid, a hierarchy rebuilt after a change of K, patterns in HBM and on the host -- and has to return the
    bits this process computes without it."""
    import subprocess
    import sys

    from tests.helpers.product import ROOT

    script = r'''
import importlib, os, sys
import numpy as np
sys.path.insert(0, %r)
from tests.helpers import meshes
pkg = importlib.import_module("fem-shell_amd")
out = {}
for kind in ("panel", "quads"):
    m = meshes.structured(40, 40, 0, 0, 10, 10, kind="t" if kind == "panel" else "q", ul_lr=True, bcids=(0, 0, 0, 0) if kind == "panel" else (1, 1, 1, 1), factor=300.0, loading=2)
    fs = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    u, info = fs.solve(rtol=1e-10, max_it=20000)
    out[kind + "_jacobi"] = u
    for where in ("device", "host"):
        os.environ["FEMSHELL_AMG_SYMBOLIC"] = where
        dm = m.dirichlet_mask()
        dm[m.n_nodes // 2 + (1 if where == "host" else 0)] = 0x3F   # K changes: the hierarchy is rebuilt
        fs.set_dirichlet(dm)
        fs.set_preconditioner("amg", coarsest_nodes=60)
        u, info = fs.solve(rtol=1e-10, max_it=500)
        assert info["converged"] == 1
        out[kind + "_amg_" + where] = u
        out[kind + "_hist_" + where] = fs.residual_history()
    fs.close()
np.savez(sys.argv[1], **out)
''' % (ROOT,)
    files = {}
    for name, poison in (("plain", "0"), ("poisoned", "1")):
        files[name] = str(tmp_path / (name + ".npz"))
        env = dict(os.environ, FEMSHELL_POOL_POISON=poison, FEMSHELL_AMG_DEVICE_MIN="100")
        r = subprocess.run([sys.executable, "-c", script, files[name]], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    a, b = np.load(files["plain"]), np.load(files["poisoned"])
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 10
    for k in a.files:
        assert np.isfinite(b[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
