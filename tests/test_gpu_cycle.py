"""One multigrid cycle z = M^-1 r (femshell_pc_apply) as an operator, against the restatement's amg_oracle.cycle() evaluated on the
device's own exported hierarchy (tests/helpers/cycle_ref.py).  The setup is held to the restatement level by level in
tests/test_gpu_amg.py; what these tests isolate is the solve phase -- Chebyshev smoothers, restriction and prolongation, the K
cycle's Krylov steps, the coarsest solve -- on the paths the benchmark runs: level 0 on single-precision copies, symmetric
storage of the coarse levels, k_spmv_node, the coarsest inverse in single precision.  A flexible CG around the cycle converges
for any SPD-ish preconditioner, so a wrong cycle only costs the solve a few iterations, which the iteration-count tests allow;
here the agreement is held to rounding.

Tolerances (tests/helpers/cycle_ref.py; relative 2-norm of z - z_ref, and the worst node's error against the largest node of
z_ref), with the largest values measured on an MI355X over every case below:
  TOL_FP64  FP64 levels: the two evaluations differ in summation order only.  Random vectors 6e-16; the load vector, smooth, up
            to 7.7e-13 (K cycle, symmetric coarse levels): its correction lives on the coarse levels, where the K cycle's
            coefficients are ratios of dot products that cancel.  5e-12.
  TOL_F32   single-precision copies of the values (FEMSHELL_AMG_VEC_F32=0) against the float model: 1.0e-12 (the device's own
            block-Jacobi inverse rounds to a float like numpy's); 1e-11.  The same runs differ from the all-FP64 reference by
            3.2e-8 at least -- the float path ran.
  TOL_VEC   FEMSHELL_AMG_VEC_F32=1/2 against the same values-only model: the products' results (and, with 2, the Chebyshev
            direction) are rounded to float besides, a relative 2^-24 = 6e-8 per product and entry, through the degree-3/4
            polynomials and the coarse correction: 6.5e-7 relative, 1.7e-6 on the worst node (load vector); 5e-6.  That the
            vector rounding ran shows as a distance of at least 100 x TOL_F32 from the values-only model (3.8e-8 measured), where
            the same context with FEMSHELL_AMG_VEC_F32=0 sits at 1e-12.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import cycle_ref, meshes
from tests.helpers.product import ROOT, ensure_built, pkg

pytestmark = pytest.mark.gpu

TOL_FP64, TOL_F32, TOL_VEC = cycle_ref.TOL_FP64, cycle_ref.TOL_F32, cycle_ref.TOL_VEC


def _mesh(kind, n):
    if kind == "panel":
        m = meshes.structured(n, n, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(0, 0, 0, 0), factor=300.0, loading=2)
        return m.xyz, m.tri, None, m.dirichlet_mask(), m.loads, (0.3, 1e7, 0.5)
    if kind == "cylinder":
        m = meshes.pinched_cylinder(n, n)
        return m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads, m.material
    if kind in ("quads", "mixed"):
        m = meshes.structured(n, n, 0, 0, 10, 10, kind="q", bcids=(1, 1, 1, 1), factor=300.0, loading=2)
        if kind == "quads":
            return m.xyz, None, m.quad, m.dirichlet_mask(), m.loads, (0.3, 1e7, 0.5)
        half = len(m.quad) // 2
        tri = np.concatenate([m.quad[half:, [0, 1, 2]], m.quad[half:, [0, 2, 3]]]).astype(np.int32)
        return m.xyz, tri, m.quad[:half], m.dirichlet_mask(), m.loads, (0.3, 1e7, 0.5)
    if kind == "strip":  # clamped all round: a third of the nodes Dirichlet
        m = meshes.structured(n, 6, 0, 0, 16.0, 1.0, kind="t", ul_lr=True, bcids=(1, 1, 1, 1), factor=300.0, loading=2)
        return m.xyz, m.tri, None, m.dirichlet_mask(), m.loads, (0.3, 1e7, 0.05)
    if kind == "delaunay":  # test_gpu_amg.py test_restriction_rows_wider_than_the_lds_panel: a level-1 row of 162 fine nodes
        from tests.test_gpu_parity import delaunay_shell
        xyz, tri = delaunay_shell(n, 5)
        dmask = np.zeros(len(xyz), dtype=np.uint8)
        dmask[xyz[:, 0] < 0.2] = 0x3F
        return xyz, tri, None, dmask, np.random.default_rng(3).normal(size=(len(xyz), 6)), (0.3, 7.0e4, 0.03)
    if kind == "poor":  # test_gpu_amg.py test_patch_smoother_on_a_shell_of_poor_element_quality_follows_the_restatement
        from tests.test_gpu_amg import _poor_shell
        xyz, tri, dmask, loads = _poor_shell(n, 2)
        return xyz, tri, None, dmask, loads, (0.3, 7.0e4, 0.03)
    raise ValueError(kind)


def _context(kind, n, cycle="K", coarsest_nodes=60, flags=pkg.REF_DEFAULT):
    ensure_built()
    xyz, tri, quad, dmask, loads, mat = _mesh(kind, n)
    fs = pkg.FemShell(*mat, flags=flags, device=0)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.assemble()
    fs.set_preconditioner("amg", cycle=cycle, coarsest_nodes=coarsest_nodes)
    return fs


def _vectors(fs):
    """The two inputs of every case: a random vector and the load vector F (smooth)."""
    r = np.random.default_rng(11).standard_normal(6 * fs.n_nodes) * cycle_ref.free_dofs(fs)
    return {"random": r, "load": fs.export_bsr()[3]}


def _report(name, **values):
    print("[cycle] %-48s %s" % (name, " ".join("%s=%.3e" % kv for kv in values.items())))


def _check_against_reference(fs, name, kcycle, float_mode, tol, fp64_gap=False, patch=False):
    """pc_apply on both vectors against the reference (float_mode: FEMSHELL_AMG_SMOOTH_F32 of the context); fp64_gap: the device
    must also differ from the all-FP64 reference by 20 x tol at least, or nothing shows that the float path ran.
    Returns {vector name: z}."""
    vecs = _vectors(fs)
    zs = {v: fs.pc_apply(r) for v, r in vecs.items()}
    levels, perm = cycle_ref.levels_from_context(fs, float_mode=float_mode)
    if float_mode and not patch:
        assert any(hasattr(L, "As") for L in levels), "no level of this case keeps single-precision copies"
    if fp64_gap:
        levels64, _ = cycle_ref.levels_from_context(fs, float_mode=0)
    for v, r in vecs.items():
        rel, node = cycle_ref.errors(zs[v], cycle_ref.apply(levels, r, kcycle, perm))
        gap = cycle_ref.errors(zs[v], cycle_ref.apply(levels64, r, kcycle, perm))[0] if fp64_gap else float("nan")
        _report(name + ":" + v, rel=rel, node=node, gap64=gap, tol=tol)
        assert rel <= tol and node <= tol, (name, v, rel, node, tol)
        if tol == TOL_VEC:  # (the vectors were rounded: away from the values-only model, where FEMSHELL_AMG_VEC_F32=0 sits at 1e-12)
            assert rel >= 100.0 * TOL_F32, (name, v, rel)
        if fp64_gap:
            assert gap >= 20.0 * tol, (name, v, gap, tol)
    return zs


def _properties(fs, name, kcycle, symmetric_tol=None):
    """Reference-free properties: the same bits twice (the last-workgroup reductions of the K cycle), M(2r) = 2 M(r) bit for bit,
    and for the V cycle x.M y = y.M x and x.M x > 0."""
    vecs = _vectors(fs)
    x = vecs["random"]
    z1 = fs.pc_apply(x)
    np.testing.assert_array_equal(fs.pc_apply(x), z1)
    np.testing.assert_array_equal(fs.pc_apply(2.0 * x), 2.0 * z1)
    if symmetric_tol is not None:
        y = np.random.default_rng(12).standard_normal(len(x)) * cycle_ref.free_dofs(fs)
        My = fs.pc_apply(y)
        xMy, yMx = x @ My, y @ z1
        scale = np.sqrt((x @ z1) * (y @ My))
        asym = abs(xMy - yMx) / scale
        _report(name + ":symmetry", asym=asym, tol=symmetric_tol)
        assert x @ z1 > 0.0 and y @ My > 0.0
        assert asym <= symmetric_tol, (name, asym)


# (name, mesh, size, environment, cycles, SMOOTH_F32 mode the reference models, tolerance, float path must show)
F64 = {"FEMSHELL_AMG_SMOOTH_F32": "0"}
CASES = [
    # level 0 above 4096 nodes: the production rules (mode 1) put level 0 on float copies
    ("panel72-fp64", "panel", 72, F64, "VK", 0, TOL_FP64, False),
    ("panel72-f32-vec0", "panel", 72, {"FEMSHELL_AMG_VEC_F32": "0"}, "VK", 1, TOL_F32, True),
    ("panel72-f32-default", "panel", 72, {}, "K", 1, TOL_VEC, False),
    ("panel72-f32all-vec0", "panel", 72, {"FEMSHELL_AMG_SMOOTH_F32": "3", "FEMSHELL_AMG_VEC_F32": "0"}, "VK", 3, TOL_F32, True),
    ("panel72-f32all-vec1", "panel", 72, {"FEMSHELL_AMG_SMOOTH_F32": "3", "FEMSHELL_AMG_VEC_F32": "1"}, "K", 3, TOL_VEC, False),
    ("panel72-f32lvl0-vec0", "panel", 72, {"FEMSHELL_AMG_SMOOTH_F32": "2", "FEMSHELL_AMG_VEC_F32": "0"}, "K", 2, TOL_F32, True),
    # symmetric storage of every coarse level against full storage
    ("panel72-sym-fp64", "panel", 72, dict(F64, FEMSHELL_AMG_COARSE_SYM="1"), "VK", 0, TOL_FP64, False),
    ("panel72-sym-f32all-vec0", "panel", 72, {"FEMSHELL_AMG_COARSE_SYM": "1", "FEMSHELL_AMG_SMOOTH_F32": "3", "FEMSHELL_AMG_VEC_F32": "0"},
     "VK", 3, TOL_F32, True),
    ("panel72-sym-f32all-vec2", "panel", 72, {"FEMSHELL_AMG_COARSE_SYM": "1", "FEMSHELL_AMG_SMOOTH_F32": "3", "FEMSHELL_AMG_VEC_F32": "2"},
     "K", 3, TOL_VEC, False),
    ("cylinder64-fp64", "cylinder", 64, F64, "K", 0, TOL_FP64, False),
    ("cylinder64-f32-vec0", "cylinder", 64, {"FEMSHELL_AMG_VEC_F32": "0"}, "K", 1, TOL_F32, True),
    ("quads40-fp64", "quads", 40, F64, "K", 0, TOL_FP64, False),
    ("mixed40-fp64", "mixed", 40, F64, "K", 0, TOL_FP64, False),
    ("strip96-fp64", "strip", 96, F64, "VK", 0, TOL_FP64, False),
    # 2401 nodes: the last slice of level 0 holds one node
    ("panel48-fp64", "panel", 48, F64, "VK", 0, TOL_FP64, False),
    ("panel48-f32all-vec0", "panel", 48, {"FEMSHELL_AMG_SMOOTH_F32": "3", "FEMSHELL_AMG_VEC_F32": "0"}, "V", 3, TOL_F32, True),
    # kernel variants that a context reads at setup or per call
    ("panel48-unfused-cheb", "panel", 48, dict(F64, FEMSHELL_AMG_FUSED_CHEB="0"), "K", 0, TOL_FP64, False),
    ("panel48-diag-full", "panel", 48, dict(F64, FEMSHELL_DIAG_UPPER="0"), "K", 0, TOL_FP64, False),
    ("panel48-device-galerkin", "panel", 48, dict(F64, FEMSHELL_AMG_DEVICE_MIN="100"), "K", 0, TOL_FP64, False),
    ("panel48-device-galerkin-sym", "panel", 48, dict(F64, FEMSHELL_AMG_DEVICE_MIN="100", FEMSHELL_AMG_COARSE_SYM="1"), "K", 0, TOL_FP64, False),
    ("panel48-no-increments", "panel", 48, dict(F64, FEMSHELL_AMG_RESIDUAL_INCREMENT="0"), "K", 0, TOL_FP64, False),
]


@pytest.mark.parametrize("name,kind,n,env,cycles,mode,tol,gap", CASES, ids=[c[0] for c in CASES])
def test_one_cycle_equals_the_restatement_on_the_exported_hierarchy(monkeypatch, name, kind, n, env, cycles, mode, tol, gap):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for cyc in cycles:
        fs = _context(kind, n, cycle=cyc)
        _check_against_reference(fs, name + "-" + cyc, cyc == "K", mode, tol, fp64_gap=gap)
        # (symmetric where nothing rounds vectors: FP64 levels, or float copies of the values with FEMSHELL_AMG_VEC_F32=0)
        sym = TOL_FP64 if cyc == "V" and (mode == 0 or env.get("FEMSHELL_AMG_VEC_F32") == "0") else None
        _properties(fs, name + "-" + cyc, cyc == "K", sym)
        fs.close()


def test_morton_numbered_delaunay_shell_with_rows_wider_than_the_lds_panel(monkeypatch):
    """FEMSHELL_REORDER_MORTON: pc_apply takes and returns the caller's numbering; the reference runs in the internal one, read off
    the diagonal blocks.  The mesh's restriction onto the coarsest level has a row of 162 fine nodes (k_spmv's passes over 64 LDS
    slots at a time).  The slivers on the hull make K ill-conditioned (kappa ~ 1e13, test_gpu_amg.py): rounding differences of the
    two evaluations grow with it -- 4.1e-12 relative, 5.9e-12 on the worst node for the random vector -- so 1e-10 here."""
    monkeypatch.setenv("FEMSHELL_AMG_PATCH_TAU", "0")
    monkeypatch.setenv("FEMSHELL_AMG_SMOOTH_F32", "0")
    fs = _context("delaunay", 2500, cycle="K", coarsest_nodes=200, flags=pkg.REF_DEFAULT | pkg.REORDER_MORTON)
    _check_against_reference(fs, "delaunay-morton-K", True, 0, 1e-10)
    levels, perm = cycle_ref.levels_from_context(fs)
    assert perm is not None and len(levels) >= 3
    assert np.diff(levels[-2].R.tocsr().indptr).max() // 6 > 64  # (a restriction row of more than 64 fine nodes: wider than the LDS panel)
    _properties(fs, "delaunay-morton-K", True)
    fs.close()


def test_patch_smoother_cycle_on_the_poor_quality_shell():
    """Level 0 smooths with one block per cluster of rigidly coupled nodes (csrc/amg_patch.hpp).  The reference inverts the
    clusters' diagonal blocks with numpy, the library with its own factorisation; on nodes a hundredth of the mesh width apart those
    blocks have condition numbers of 1e8 and beyond, so the two agree to about 1e-8 relative -- the tolerance of
    test_patch_smoother_on_a_shell_of_poor_element_quality_follows_the_restatement for P (2e-6) applies (measured: 1.5e-7
    relative, 3.8e-7 on the worst node)."""
    fs = _context("poor", 3000, cycle="K", coarsest_nodes=1400)
    zs = _check_against_reference(fs, "poor-shell-K", True, 1, 2e-6, patch=True)
    assert fs.amg_patch_info()["clusters"] > 500
    _properties(fs, "poor-shell-K", True)
    fs.close()
    assert all(np.all(np.isfinite(z)) for z in zs.values())


@pytest.mark.parametrize("device_min,f32", [("100000", "0"), ("0", "0"), ("0", "1")])
@pytest.mark.parametrize("cycle", ["V", "K"])
def test_coarsest_solve_host_and_device_fp64_and_float(monkeypatch, device_min, f32, cycle):
    """The coarsest inverse on the host (FP64) or on the matrix cores, FP64 or stored as floats (FEMSHELL_AMG_DENSE_F32): the
    cycle applies whichever femshell_amg_export hands out as coarse_inverse (floats widened), so the reference models it exactly."""
    monkeypatch.setenv("FEMSHELL_AMG_SMOOTH_F32", "0")
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_DEVICE_MIN", device_min)
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_F32", f32)
    fs = _context("panel", 48, cycle=cycle, coarsest_nodes=300)
    _check_against_reference(fs, "coarsest-%s-%s-%s" % (device_min, f32, cycle), cycle == "K", 0, TOL_FP64)
    st = fs.amg_dense_stats()
    assert (st["n"] > 0) == (device_min == "0")
    if f32 == "1":
        inv = fs.amg_export(len(fs.amg_levels()) - 1)["coarse_inverse"]
        np.testing.assert_array_equal(inv, inv.astype(np.float32).astype(np.float64))
    fs.close()


def test_fused_starts_give_the_bits_of_the_separate_passes(monkeypatch):
    """FEMSHELL_AMG_FUSE bit 1 (k_sym_gather_start_node, symmetric-storage levels) repeats the arithmetic of k_sym_gather_node + k_cheb_start_node
    bit for bit (csrc/amg_solve.cpp fuse_mask); bit 0 (k_pcg_update_start_node) is not on pc_apply's path.  Bit 2 (the epilogue of
    k_spmv on full-storage levels) rounds x + c z as one multiply-add: the reference's tolerance, not the same bits."""
    monkeypatch.setenv("FEMSHELL_AMG_COARSE_SYM", "1")
    for mode, vec in (("0", "0"), ("3", "2")):
        monkeypatch.setenv("FEMSHELL_AMG_SMOOTH_F32", mode)
        monkeypatch.setenv("FEMSHELL_AMG_VEC_F32", vec)
        got = {}
        for fuse in ("0", "3", "-1"):
            monkeypatch.setenv("FEMSHELL_AMG_FUSE", fuse)
            fs = _context("panel", 48)
            got[fuse] = _check_against_reference(fs, "fuse%s-f32%s" % (fuse, mode), True, int(mode), TOL_FP64 if mode == "0" else TOL_VEC)
            fs.close()
        for v in got["0"]:
            np.testing.assert_array_equal(got["0"][v], got["3"][v])
    monkeypatch.setenv("FEMSHELL_AMG_COARSE_SYM", "100000")
    monkeypatch.setenv("FEMSHELL_AMG_SMOOTH_F32", "0")
    for fuse in ("0", "-1"):  # (full-storage coarse levels: bit 2 takes the start into k_spmv's epilogue)
        monkeypatch.setenv("FEMSHELL_AMG_FUSE", fuse)
        fs = _context("panel", 48)
        _check_against_reference(fs, "fuse%s-full" % fuse, True, 0, TOL_FP64)
        fs.close()


def _worker(tmp_path, name, env):
    out = str(tmp_path / (name + ".npz"))
    e = dict(os.environ, **env)
    subprocess.run([sys.executable, "-m", "tests.helpers.cycle_worker", out], cwd=ROOT, env=e, check=True, timeout=300)
    return np.load(out)


def test_kernel_choices_a_process_reads_once(tmp_path):
    """FEMSHELL_SPMV_NODE_WIDTH and FEMSHELL_SPMV_CHUNK are read once per process: each setting runs in a
    child process (tests/helpers/cycle_worker.py) and is held to the reference there.  k_spmv_node sums every row in the order
    k_spmv does -- 'same bits' (csrc/spmv_kernels.hip) --: width 0 (never k_spmv_node) and 1000 (every full-storage product) against the
    default give the same z."""
    base = _worker(tmp_path, "default", {})
    runs = {"width0": {"FEMSHELL_SPMV_NODE_WIDTH": "0"},
            "width1000": {"FEMSHELL_SPMV_NODE_WIDTH": "1000"}, "chunk1": {"FEMSHELL_SPMV_CHUNK": "1"},
            "chunk2": {"FEMSHELL_SPMV_CHUNK": "2"}, "chunk4": {"FEMSHELL_SPMV_CHUNK": "4"}}
    for name, env in [("default", {})] + list(runs.items()):
        got = base if name == "default" else _worker(tmp_path, name, env)
        err = got["err"]
        _report("worker-" + name, rel=err[:, 0].max(), node=err[:, 1].max(), same_bits=float(np.array_equal(got["z"], base["z"])))
        assert int(got["levels"]) >= 3
        assert err.max() <= TOL_FP64, (name, err)
        if name.startswith("width"):
            np.testing.assert_array_equal(got["z"], base["z"])
            np.testing.assert_array_equal(got["zF"], base["zF"])


def test_pc_apply_leaves_the_next_solve_alone():
    """A solve after pc_apply gives the bits of a solve without it -- in a fresh context (pc_apply builds the hierarchy) and between
    two solves of one context (pc_apply reuses it); and pc_apply behind a solve (the CG's scalars finished, the workspaces full)
    gives the bits of pc_apply in a fresh context."""
    fs = _context("panel", 48)
    u0, i0 = fs.solve(rtol=1e-10, max_it=400)
    h0 = fs.residual_history()
    r = np.random.default_rng(5).standard_normal(6 * fs.n_nodes) * cycle_ref.free_dofs(fs)
    z_after_solve = fs.pc_apply(r)
    u1, i1 = fs.solve(rtol=1e-10, max_it=400)
    assert i0["iterations"] == i1["iterations"] and i1["pc_setup_seconds"] == 0.0
    np.testing.assert_array_equal(u0, u1)
    np.testing.assert_array_equal(h0, fs.residual_history())
    fs.close()
    fs = _context("panel", 48)
    np.testing.assert_array_equal(fs.pc_apply(r), z_after_solve)
    assert len(fs.amg_levels()) >= 3
    u2, i2 = fs.solve(rtol=1e-10, max_it=400)
    assert i2["iterations"] == i0["iterations"]
    np.testing.assert_array_equal(u0, u2)
    np.testing.assert_array_equal(h0, fs.residual_history())
    fs.close()


def test_pc_apply_with_block_jacobi_is_unsupported():
    ensure_built()
    xyz, tri, quad, dmask, loads, mat = _mesh("panel", 8)
    fs = pkg.FemShell(*mat, device=0)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.set_preconditioner("jacobi")
    with pytest.raises(pkg.FemShellError) as e:
        fs.pc_apply(np.ones(6 * fs.n_nodes))
    assert e.value.code == -7  # FEMSHELL_ERR_UNSUPPORTED
    fs.close()


# ---- the dense coarsest inverse at the edges of its tiles ---------------------------------------------------------------------

@pytest.mark.parametrize("cells", [2, 7, 9, 10, 13])  # 9, 64, 100, 121, 196 nodes: K itself is the coarsest operator
@pytest.mark.parametrize("tile", ["64", "128"])
@pytest.mark.parametrize("f32", ["0", "1"])
def test_dense_inverse_at_tile_edges(monkeypatch, cells, tile, f32):
    """csrc/amg_dense.hip at exact sizes: 9 nodes (54 dofs, less than one 64-tile), 64 nodes (384 dofs: a multiple of 64 and of
    128), 100, 121, 196 nodes.  The inverse the matrix cores computed against numpy's inverse of the exported operator; defect
    bounds as in test_gpu_amg.py test_dense_inverse_on_the_matrix_cores_equals_the_host_inverse."""
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_DEVICE_MIN", "0")
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_TILE", tile)
    monkeypatch.setenv("FEMSHELL_AMG_DENSE_F32", f32)
    ensure_built()
    m = meshes.structured(cells, cells, 0, 0, 10, 10, kind="t", ul_lr=True, bcids=(1, 0, 0, 0), factor=300.0, loading=2)
    fs = pkg.FemShell(0.3, 1e7, 0.5, device=0)
    fs.set_mesh(m.xyz, m.tri)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    fs.set_preconditioner("amg")
    fs.assemble()
    free = cycle_ref.free_dofs(fs)
    r = np.random.default_rng(1).standard_normal(6 * m.n_nodes) * free
    z = fs.pc_apply(r)
    lv = fs.amg_levels()
    assert len(lv) == 1 and lv[0]["n_nodes"] == (cells + 1) ** 2
    ex = fs.amg_export(0)
    A = cycle_ref.bsr(ex["A_rowptr"], ex["A_cols"], ex["A_vals"], m.n_nodes).toarray()
    inv = ex["coarse_inverse"]
    st = fs.amg_dense_stats()
    assert st["n"] == 6 * m.n_nodes and st["dropped_directions"] == 0
    ref = np.linalg.inv(A)
    defect = np.abs(A @ inv - np.eye(len(A))).max()
    f = np.ix_(free, free)  # (the Dirichlet rows' unit entries would dominate the norms)
    rel = np.linalg.norm(inv[f] - ref[f]) / np.linalg.norm(ref[f])
    zrel = np.linalg.norm(z - inv @ r) / np.linalg.norm(inv @ r)
    _report("dense-%d-%s-%s" % (m.n_nodes, tile, f32), defect=defect, rel=rel, apply=zrel)
    assert defect <= (1e-9 if f32 == "0" else 2e-4), defect  # (measured: 2.7e-13 / 9.4e-6 at 196 nodes)
    assert rel <= (1e-12 if f32 == "0" else 1e-7), rel  # (measured: 1.3e-17 / 2.8e-8)
    assert zrel <= TOL_FP64, zrel  # (the cycle of a one-level hierarchy is the product with that inverse; measured 8e-20)
    fs.close()


# ---- the row-partitioned cycle (two and three ranks on one GPU over the test transport, tests/test_multirank_gpu.py) -----------

@pytest.mark.parametrize("world,kind,dist_min,f32", [(2, "panel", 100, False), (3, "panel", 100, False), (3, "cylinder", 60000, False),
                                                     (2, "panel", 100, True)])
def test_row_partitioned_cycle_equals_the_restatement(world, kind, dist_min, f32, tmp_path):
    """pc_apply on a row-partitioned context: every rank passes and gets back its owned rows (after a solve), the halo products of
    the split levels, restriction and prolongation across the cuts, the all-reduced K-cycle coefficients and the all-gather onto
    the replicated levels run.  The ranks' z put together against cycle() on the levels the ranks export -- the split levels'
    rows one under the other, the replicated ones from one rank.  dist_min = 100: levels 0 and 1 are split.  f32: every level on
    single-precision copies (FEMSHELL_AMG_SMOOTH_F32=3; split levels keep FP64 vectors), held to the float model.  Measured: FP64
    1.6e-13 on the worst node, float model 1.1e-13, and 1.8e-6 between the float run and the FP64 reference."""
    import scipy.sparse as sp
    from tests.test_multirank_gpu import run_ranks

    env = {"FEMSHELL_AMG_DIST_MIN": str(dist_min), "FEMSHELL_TEST_AMG_EXPORT": "1", "FEMSHELL_TEST_EXPORT": "1",
           "FEMSHELL_TEST_PC_APPLY": "1", "FEMSHELL_AMG_SMOOTH_F32": "3" if f32 else "0", "FEMSHELL_AMG_VEC_F32": "0"}
    ranks = sorted(run_ranks(world, kind, tmp_path, pc="amg", extra_env=env), key=lambda q: int(q["begin"]))
    n_nodes = [int(v) for v in ranks[0]["amg_n_nodes"]]
    d = int(ranks[0]["amg_partitioned_levels"])
    assert d == (2 if dist_min == 100 else 1) and len(n_nodes) >= d + 1  # (the last split level restricts onto a replicated one)
    n = n_nodes[0]

    def stack(level, what, nc):
        rp, ci, va = [np.zeros(1, dtype=np.int64)], [], []
        for r in ranks:
            p = np.asarray(r["amg_L%d_%s_rowptr" % (level, what)], dtype=np.int64)
            rp.append(p[1:] + rp[-1][-1])
            ci.append(r["amg_L%d_%s_cols" % (level, what)])
            va.append(r["amg_L%d_%s_vals" % (level, what)].reshape(-1, 6, 6))
        return cycle_ref.bsr(np.concatenate(rp), np.concatenate(ci), np.concatenate(va), nc)

    def whole(level, what, nc):
        r = ranks[-1]
        return cycle_ref.bsr(r["amg_L%d_%s_rowptr" % (level, what)], r["amg_L%d_%s_cols" % (level, what)], r["amg_L%d_%s_vals" % (level, what)], nc)

    # level 0: K as the ranks assembled it
    off = np.cumsum([0] + [int(np.asarray(r["k_rowptr"])[-1]) for r in ranks])
    rp = np.concatenate([[0]] + [np.asarray(r["k_rowptr"], dtype=np.int64)[1:] + off[i] for i, r in enumerate(ranks)])
    ci = np.concatenate([r["k_cols"][:int(np.asarray(r["k_rowptr"])[-1])] for r in ranks])
    va = np.concatenate([r["k_vals"][:int(np.asarray(r["k_rowptr"])[-1])].reshape(-1, 6, 6) for r in ranks])
    As = [sp.bsr_matrix((va, ci, rp), shape=(6 * n, 6 * n))]
    Ps = []
    for li in range(len(n_nodes)):
        if li > 0:
            As.append(stack(li, "A", n_nodes[li]) if li < d else whole(li, "A", n_nodes[li]))
        if li + 1 < len(n_nodes):
            Ps.append(stack(li, "P", n_nodes[li + 1]) if li < d else whole(li, "P", n_nodes[li + 1]))
    inv = ranks[-1]["amg_L%d_coarse_inverse" % (len(n_nodes) - 1)]
    lams = [float(v) for v in ranks[0]["amg_lambda"]]
    levels = cycle_ref.build_levels(As, Ps, lams, inv, float_mode=3 if f32 else 0)
    tol = TOL_F32 if f32 else TOL_FP64
    vecs = {"random": (ranks[0]["pc_r"].ravel(), "pc_z"), "load": (np.concatenate([r["pc_F"] for r in ranks]), "pc_zF")}
    for v, (rvec, key) in vecs.items():
        z = np.zeros((n, 6))
        for r in ranks:
            z[r["own"]] = r[key].reshape(-1, 6)
        rel, node = cycle_ref.errors(z.ravel(), cycle_ref.apply(levels, rvec, True))
        gap = float("nan")
        if f32:
            gap = cycle_ref.errors(z.ravel(), cycle_ref.apply(cycle_ref.build_levels(As, Ps, lams, inv), rvec, True))[0]
        _report("dist-%d-%s-%d-%s:%s" % (world, kind, dist_min, "f32" if f32 else "fp64", v), rel=rel, node=node, gap64=gap, tol=tol)
        assert rel <= tol and node <= tol, (v, rel, node, tol)
        if f32:
            assert gap >= 20.0 * tol, (v, gap)

