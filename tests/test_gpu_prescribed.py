"""Prescribed displacements, support reactions and the matrix-free product with the unconstrained stiffness
(femshell_set_prescribed, femshell_reactions, femshell_element_product) against tests/helpers/prescribed.py."""
import functools

import numpy as np
import pytest

from tests.helpers import meshes, oracle, prescribed as pr, sections
from tests.helpers.product import ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

TINY = 1e-12  # the block-wise tolerance the project holds K to (tests/test_gpu_parity.py), carried through the product


def rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


# ------------------------------------------------------------------ 1. the product against the oracle

def product_bound_ratio(y, y_ref, K_unc, x):
    """max over the node rows a of max|y - y_ref| / (1e-12 S_a): the bound of test_element_product_matches_the_oracle is 1"""
    return (np.abs(y - y_ref).reshape(-1, 6).max(axis=1) / (TINY * pr.row_scale(K_unc, x))).max()


def _product_meshes():
    one = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], dtype=np.float64), np.array([[0, 1, 2]], np.int32), None)
    two = (np.array([[0, 0, 0], [1, 0, 0.1], [1, 1, 0], [0, 1, 0.2]], dtype=np.float64), np.array([[0, 1, 2], [0, 2, 3]], np.int32), None)
    lifted = pr.panel(lift=True)
    return {
        "one_triangle": lambda: one,
        "two_triangles": lambda: two,
        "strip33": lambda: pr.strip33() + (None,),
        "lifted_panel": lambda: lifted + (None,),
        "mixed_petals24": lambda: meshes.mixed_petals(24),
        "coil300": lambda: meshes.coil(300) + (None,),
        "delaunay600_rcm": lambda: meshes.delaunay_patch(600, 2, strips=False) + (None,),
        "panel_three_sections": lambda: lifted + (None,),
        "lifted_panel_full_storage": lambda: lifted + (None,),
    }


@pytest.mark.parametrize("name", list(_product_meshes()))
def test_element_product_matches_the_oracle(name, monkeypatch):
    """max|y - y_ref| <= 1e-12 S_a per node row, S_a = sum_b max|K_ab| ||x_b||_1; two calls give the same bits.
    (the rounding of a row sum, about 6 (blocks in the row) eps, is two orders below the bound)"""
    xyz, tri, quad = _product_meshes()[name]()
    if name == "delaunay600_rcm":
        monkeypatch.setenv("FEMSHELL_REORDER", "rcm")
    if name == "lifted_panel_full_storage":
        monkeypatch.setenv("FEMSHELL_SYMMETRIC", "0")
    fs = pkg.FemShell(pr.NU, pr.E, pr.T)
    fs.set_mesh(xyz, tri, quad)
    sec = None
    if name == "panel_three_sections":
        sec = (sections.THREE, sections.strips_of(xyz, tri), None)
        fs.set_sections(sec[0], sec[1], None)
    if name == "coil300":
        assert fs.assembly_kernel() == "k_assemble"  # a slice list far beyond what the pipelined kernel takes
    # a Dirichlet set must not show in the product
    mask = np.zeros(len(xyz), np.uint8)
    mask[::3] = 0x15
    fs.set_dirichlet(mask)
    x = np.random.default_rng(7).uniform(-1.0, 1.0, 6 * len(xyz))
    y = fs.element_product(x)
    assert np.array_equal(y, fs.element_product(x))
    K_unc, _ = pr.matrices(xyz, tri, quad, oracle.material(pr.NU, pr.E, pr.T), np.zeros(len(xyz), np.uint8), sec)
    y_ref = oracle.spmv(*K_unc, x)
    ratio = product_bound_ratio(y, y_ref, K_unc, x)
    print("element_product_vs_oracle %-28s nodes %5d  max |y - y_ref| / (1e-12 S_a) = %.3e" % (name, len(xyz), ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------ 2. prescribed solves against the reference

def _case(name):
    """(xyz, tri, quad, thickness, mask, ubar, loads)"""
    if name == "membrane_patch":
        xyz, tri, mask, ubar, _ = pr.membrane_patch()
        return xyz, tri, None, pr.T, mask, ubar, None
    if name in ("cantilever_t0.37", "cantilever_t0.05"):
        xyz, tri, mask, ubar, _ = pr.cantilever()
        return xyz, tri, None, float(name.split("_t")[1]), mask, ubar, None
    if name == "supported_plate":
        xyz, tri, mask, ubar = pr.supported_plate()
        return xyz, tri, None, pr.T, mask, ubar, None
    assert name == "mixed_moved_edge"
    xyz, tri, quad, mask, ubar = pr.mixed_moved_edge()
    return xyz, tri, quad, pr.T, mask, ubar, None


CASES = ["membrane_patch", "cantilever_t0.37", "cantilever_t0.05", "supported_plate", "mixed_moved_edge"]


@functools.lru_cache(maxsize=None)
def _reference(name):
    xyz, tri, quad, t, mask, ubar, loads = _case(name)
    return pr.Reference(xyz, tri, quad, oracle.material(pr.NU, pr.E, t), mask, loads, ubar)


def _context(xyz, tri, quad, t, mask, ubar=None, loads=None, pc="jacobi"):
    fs = pkg.FemShell(pr.NU, pr.E, t)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(mask)
    if loads is not None:
        fs.set_loads(loads)
    if ubar is not None:
        fs.set_prescribed(ubar)
    if pc == "amg":
        fs.set_preconditioner("amg")
    return fs


@functools.lru_cache(maxsize=None)
def _solved(name, pc):
    xyz, tri, quad, t, mask, ubar, loads = _case(name)
    fs = _context(xyz, tri, quad, t, mask, ubar, loads, pc)
    u, info = fs.solve(rtol=1e-13, max_it=50000)
    return fs, u, info


@pytest.mark.parametrize("pc", ["jacobi", "amg"])
@pytest.mark.parametrize("name", CASES)
def test_prescribed_solve_matches_the_reference(name, pc):
    ref = _reference(name)
    fs, u, info = _solved(name, pc)
    err = rel(u, ref.u)
    print("prescribed solve %-18s %-6s iterations %5d  error vs reference %.2e" % (name, pc, info["iterations"], err))
    assert info["converged"] == 1
    assert err <= 1e-10
    # the prescribed values at the fixed dofs, bit for bit
    assert np.array_equal(u.ravel()[ref.fixed], ref.ubar[ref.fixed])
    assert np.array_equal(fs.get_solution(), u)
    if name == "membrane_patch":  # the closed form
        exact = pr.membrane_patch()[4]
        assert np.abs(u - exact).max() <= 1e-10 * np.abs(exact).max()


# ------------------------------------------------------------------ 3. rigid translation

@pytest.mark.parametrize("pc", ["jacobi", "amg"])
def test_rigid_translation_moves_every_node_and_loads_no_support(pc):
    ref = _reference("mixed_moved_edge")
    fs, u, _ = _solved("mixed_moved_edge", pc)
    move = np.array([1e-3, 2e-3, 3e-3, 0.0, 0.0, 0.0])
    err = np.abs(u - move).max() / np.abs(move).max()
    r = fs.reactions()
    S = ref.scale(u)
    print("rigid translation %-6s: displacement error %.2e, max |r| / max S_a = %.2e" % (pc, err, np.abs(r).max() / S.max()))
    assert err <= 1e-10
    # ten times the displacement tolerance: K applied to an error of that size is bounded by the scale
    assert np.abs(r).max() <= 1e-9 * S.max()


# ------------------------------------------------------------------ 4. reactions

def test_reactions_of_a_clamped_panel_under_nodal_loads():
    xyz, tri = pr.panel()
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    rng = np.random.default_rng(3)
    loads = np.zeros((n, 6))
    loads[:, :3] = rng.normal(size=(n, 3)) * [5.0, 5.0, 0.5]  # in-plane and transverse
    fs = _context(xyz, tri, None, pr.T, mask, None, loads)
    u, info = fs.solve(rtol=1e-12, max_it=50000)
    assert info["converged"] == 1
    r = fs.reactions()
    ref = pr.Reference(xyz, tri, None, oracle.material(pr.NU, pr.E, pr.T), mask, loads, None)
    r_ref = pr.reactions(ref.K_unc, u, loads)  # from the device's own u
    S = ref.scale(u)
    ratio = (np.abs(r - r_ref).max(axis=1) / (TINY * S)).max()
    free = ~ref.fixed
    F = np.where(ref.fixed, 0.0, loads.ravel())
    balance = np.abs(r[:, :3].sum(axis=0) + loads[:, :3].sum(axis=0)).max()
    print("reactions: |r - r_ref| / (1e-12 S_a) = %.2e, free dofs |r| / |F| = %.2e, force balance / (1e-12 sum S_a) = %.2e"
          % (ratio, np.linalg.norm(r.ravel()[free]) / np.linalg.norm(F), balance / (TINY * S.sum())))
    assert ratio <= 1.0
    assert np.linalg.norm(r.ravel()[free]) <= 1e-9 * np.linalg.norm(F)
    # the translations are in the null space of K_unc: the supports carry the loads
    assert balance <= TINY * S.sum()
    assert np.array_equal(fs.reactions(u), r)
    assert np.array_equal(fs.reactions(), r)


def test_reactions_with_prescribed_values_take_the_whole_solution():
    """the NULL form adds the prescribed part in the kernel: the bits of the explicit form, and the reference's reactions"""
    ref = _reference("cantilever_t0.37")
    fs, u, _ = _solved("cantilever_t0.37", "jacobi")
    r = fs.reactions()
    assert np.array_equal(fs.reactions(u), r)
    S = ref.scale(u)
    assert (np.abs(r - pr.reactions(ref.K_unc, u, ref.loads)).max(axis=1) <= TINY * S).all()
    tip = pr.cantilever()[4]
    assert abs(r[tip, 2].sum() - ref.r[tip, 2].sum()) <= 1e-9 * abs(ref.r[tip, 2].sum())


# ------------------------------------------------------------------ 5. device-only consistency

def test_device_twin_superposition_scaling_and_ignored_entries():
    xyz, tri, mask, ubar, tip = pr.cantilever()
    n = len(xyz)
    fs, u, info = _solved("cantilever_t0.37", "jacobi")
    r = fs.reactions()
    # the twin, entirely on the device: the edge free, loaded with the reactions
    mask2 = mask.copy()
    mask2[tip] = 0
    loads2 = np.zeros((n, 6))
    loads2[tip, 2] = r[tip, 2]
    u2, info2 = _context(xyz, tri, None, pr.T, mask2, None, loads2).solve(rtol=1e-13, max_it=50000)
    assert info2["converged"] == 1
    print("device twin differs by %.2e" % rel(u2, u))
    assert rel(u2, u) <= 1e-9
    # superposition
    loads = np.zeros((n, 6))
    loads[:, 2] = np.random.default_rng(5).normal(size=n)
    both, _ = _context(xyz, tri, None, pr.T, mask, ubar, loads).solve(rtol=1e-13, max_it=50000)
    only_loads, _ = _context(xyz, tri, None, pr.T, mask, None, loads).solve(rtol=1e-13, max_it=50000)
    print("superposition differs by %.2e" % rel(only_loads + u, both))
    assert rel(only_loads + u, both) <= 1e-9
    # 2 u_bar gives 2 u
    twice, _ = _context(xyz, tri, None, pr.T, mask, 2.0 * ubar).solve(rtol=1e-13, max_it=50000)
    assert rel(twice, 2.0 * u) <= 1e-9
    # garbage on free dofs of u_bar changes no bit
    fixed = pr.fixed_dofs(mask).reshape(n, 6)
    garbage = np.where(fixed, ubar, np.random.default_rng(6).normal(size=(n, 6)) * 1e3)
    ug, _ = _context(xyz, tri, None, pr.T, mask, garbage).solve(rtol=1e-13, max_it=50000)
    assert np.array_equal(ug, u)
    # ... and the order of set_dirichlet and set_prescribed does not matter
    fo = pkg.FemShell(pr.NU, pr.E, pr.T)
    fo.set_mesh(xyz, tri)
    fo.set_prescribed(ubar)
    fo.set_dirichlet(mask)
    uo, _ = fo.solve(rtol=1e-13, max_it=50000)
    assert np.array_equal(uo, u)


@pytest.mark.parametrize("pc", ["jacobi", "amg"])
def test_warm_start_from_the_homogeneous_part(pc):
    xyz, tri, quad, t, mask, ubar, loads = _case("cantilever_t0.37")
    fs = _context(xyz, tri, quad, t, mask, ubar, loads, pc)
    u, cold = fs.solve(rtol=1e-13, max_it=50000)
    fs.set_initial_guess(None)
    uw, warm = fs.solve(rtol=1e-13, max_it=50000)
    print("warm start %-6s: %d iterations after %d, differs by %.2e" % (pc, warm["iterations"], cold["iterations"], rel(uw, u)))
    assert warm["converged"] == 1 and warm["iterations"] <= cold["iterations"]
    assert rel(uw, u) <= 1e-10
    assert np.array_equal(uw[mask != 0], u[mask != 0])


# ------------------------------------------------------------------ 6. nothing moved

def test_without_prescribed_values_nothing_moves():
    xyz, tri = pr.panel(lift=True)
    n = len(xyz)
    mask = np.zeros(n, np.uint8)
    mask[pr.edge_nodes(xyz, 0, 0.0)] = 0x3F
    mask[pr.edge_nodes(xyz, 0, pr.LX)] = 0x04
    loads = np.random.default_rng(8).normal(size=(n, 6))

    def run(how):
        fs = _context(xyz, tri, None, pr.T, mask, None, loads)
        if how == "zeros":
            fs.set_prescribed(np.zeros((n, 6)))
        if how == "cleared":
            fs.set_prescribed(np.ones((n, 6)))
            fs.set_prescribed(None)
        fs.assemble()
        F = fs.export_bsr()[3]
        u, _ = fs.solve(rtol=0.0, max_it=37)
        return F, u

    F0, u0 = run("never")
    for how in ("zeros", "cleared"):
        F, u = run(how)
        assert np.array_equal(F, F0) and np.array_equal(u, u0), how


def test_set_prescribed_keeps_k_and_the_hierarchy():
    xyz, tri, mask, ubar, _ = pr.cantilever()
    fs = _context(xyz, tri, None, pr.T, mask)
    fs.set_preconditioner("amg", coarsest_nodes=12)
    fs.assemble()
    _, _, vals0, F0 = fs.export_bsr()
    _, first = fs.solve(rtol=1e-10, max_it=1000)
    assert first["amg_levels"] >= 2 and first["pc_setup_seconds"] > 0.0
    stats0 = fs.amg_setup_stats()
    fs.set_prescribed(ubar)
    _, _, vals1, F1 = fs.export_bsr()
    assert np.array_equal(vals1, vals0)
    assert not np.array_equal(F1, F0)
    fixed = pr.fixed_dofs(mask)
    assert np.all(F1[fixed] == 0.0)
    _, second = fs.solve(rtol=1e-10, max_it=1000)
    assert second["converged"] == 1
    assert second["assemble_seconds"] == 0.0 and second["pc_setup_seconds"] == 0.0  # no second assembly, no second setup
    assert fs.amg_setup_stats() == stats0
    # export_bsr's F is the right-hand side of the reference
    ref = _reference("cantilever_t0.37")
    assert np.abs(F1 - ref.rhs).max() <= TINY * ref.scale(ref.ubar).max()


# ------------------------------------------------------------------ 7. errors

def test_refusals_leave_the_context_usable():
    xyz, tri, mask, ubar, _ = pr.cantilever()
    n = len(xyz)
    fs = _context(xyz, tri, None, pr.T, mask, ubar)
    u, _ = fs.solve(rtol=1e-12, max_it=50000)
    bad = ubar.copy()
    bad[3, 1] = np.nan
    with pytest.raises(pkg.FemShellError) as e:
        fs.set_prescribed(bad)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    with pytest.raises(pkg.FemShellError) as e:
        fs.set_prescribed(np.zeros((n - 1, 6)))
    assert e.value.code == -1 and "n_nodes" in str(e.value)
    with pytest.raises(pkg.FemShellError) as e:
        fs.set_prescribed(np.zeros((1, 6)), node_ids=[n])
    assert e.value.code == -1 and "out of range" in str(e.value)
    # the old values are in force
    u2, _ = fs.solve(rtol=1e-12, max_it=50000)
    assert np.array_equal(u2, u)
    # dynamics refuses prescribed values, and the other way round
    fs.set_density(7.8e-9)
    with pytest.raises(pkg.FemShellError) as e:
        fs.dynamics_begin(1e-3)
    assert e.value.code == -1 and "prescribed" in str(e.value)
    fs.set_prescribed(None)
    fs.dynamics_begin(1e-3)
    with pytest.raises(pkg.FemShellError) as e:
        fs.set_prescribed(ubar)
    assert e.value.code == -1 and "dynamics" in str(e.value)
    fs.dynamics_end()
    fs.set_prescribed(ubar, node_ids=None)
    u3, _ = fs.solve(rtol=1e-12, max_it=50000)
    assert rel(u3, u) <= 1e-10
    # the sparse form: unlisted nodes get 0
    tip = pr.cantilever()[4]
    fs.set_prescribed(ubar[tip], node_ids=tip)
    u4, _ = fs.solve(rtol=1e-12, max_it=50000)
    assert np.array_equal(u4, u3)


def test_row_partitioned_contexts_refuse():
    """ghost values of the prescribed displacements and a halo exchange in front of the product are a later change"""
    fs = pkg.FemShell(pr.NU, pr.E, pr.T, rank=0, world_size=2)
    for call in (lambda: fs.set_prescribed(np.zeros((1, 6)), node_ids=[0]), lambda: fs.reactions(np.zeros(0)),
                 lambda: fs.element_product(np.zeros(0))):
        with pytest.raises(pkg.FemShellError) as e:
            call()
        assert e.value.code == -7 and "single-rank" in str(e.value)


def test_time_kernel_runs_the_element_product():
    xyz, tri = pr.panel(lift=True)
    fs = pkg.FemShell(pr.NU, pr.E, pr.T)
    fs.set_mesh(xyz, tri)
    ms, nbytes = fs.time_kernel(pkg.KERNEL_ELEMENT_PRODUCT, reps=3)
    assert ms > 0.0 and nbytes > (24 + 96) * len(xyz)
