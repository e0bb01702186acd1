"""Modal analysis on the GPU (femshell_modes, femshell_spmm, femshell_modal_gram) through the C ABI, against
tests/helpers/modal.py (pinned on the CPU by tests/test_modal_cpu.py).

Bounds.  Products and Gram matrices: the standard bound of a dot product of n terms in floating point, 2 n eps sum |terms|.
Eigenvalues: |lam - lam_ref| <= 1e-8 (lam_ref + shift) -- the truncation term of a pair converged to tol = 1e-6 is tol^2 / relgap
<= 1e-12 / 0.017 = 6e-11 (0.017: the smallest relative gap among the lowest twelve modes of the 12 x 10 patch), the rounding floor
kappa eps = 5e6 * 2.2e-16 = 1e-9 at worst; scipy's LOBPCG lands at 2e-10 on these matrices.  Shapes: distance to the reference's
cluster <= 1e-3 (model tol / relgap = 6e-5)."""
import os
import subprocess

import numpy as np
import pytest

from tests.helpers import dynamics, meshes, modal, sections
from tests.helpers.product import ROOT, ensure_built

pytestmark = pytest.mark.gpu
pkg = ensure_built()

NU, E, T, RHO = 0.3, 2.1e5, 0.04, 7.8e-3
SECTION_RHO = np.array([7.8e-3, 2.7e-3, 4.4e-3])
EPS = np.finfo(np.float64).eps
TOL, N_MODES = 1e-6, 8
INVALID, BREAKDOWN = -1, -5


def context(m, pc="jacobi", bc=True, density=RHO):
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    if bc:
        fs.set_dirichlet(m.dirichlet_mask())
    if density is not None:
        fs.set_density(density)
    set_pc(fs, pc)
    return fs


def set_pc(fs, pc):
    if pc == "amg":
        fs.set_preconditioner("amg")
    elif pc == "amg_small":  # a hierarchy of more than one level on a mesh of a few hundred nodes
        fs.set_preconditioner("amg", coarsest_nodes=100)
    else:
        fs.set_preconditioner("jacobi")


class Mesh:
    def __init__(self, xyz, tri=None, quad=None, dmask=None):
        self.xyz, self.tri, self.quad = np.ascontiguousarray(xyz, dtype=np.float64), tri, quad
        self.n_nodes = len(self.xyz)
        self._dmask = np.zeros(self.n_nodes, np.uint8) if dmask is None else np.ascontiguousarray(dmask, dtype=np.uint8)

    def dirichlet_mask(self):
        return self._dmask


def free_of(dmask, n):
    return dynamics.free_dofs(dmask, n)


# ------------------------------------------------------------------ 1. the block product

def product_meshes(name):
    """(context with K assembled, Dirichlet mask)"""
    if name in ("curved", "morton", "full"):
        m = sections.curved_patch(24, 18)
        return context(m), m.dirichlet_mask()
    if name == "delaunay":
        xyz, tri = meshes.delaunay_patch(3000, 2)
        dmask = np.zeros(len(xyz), np.uint8)
        dmask[xyz[:, 0] < 0.2] = 0x3F
        dmask[::97] |= 0x07
        m = Mesh(xyz, tri, None, dmask)
        return context(m), dmask
    cs = sections.mixed_patch()
    return cs.apply(pkg.FemShell(NU, E, T), loads=False), cs.dmask


@pytest.mark.parametrize("name", ["curved", "delaunay", "mixed", "morton", "full"])
def test_block_product_meets_the_dot_product_bound(monkeypatch, name):
    """column j of spmm(X) against the float64 product of the exported BSR: |err|_i <= 2 n_i eps (|K||x|)_i, n_i = 6 x blocks in
    row i; femshell_spmv itself meets it on the same inputs.  1, 3, 4, 5, 8 columns: the tail instantiations and two passes."""
    if name == "morton":
        monkeypatch.setenv("FEMSHELL_REORDER", "morton")
    if name == "full":
        monkeypatch.setenv("FEMSHELL_SYMMETRIC", "0")
    fs, dmask = product_meshes(name)
    fs.assemble()
    r, c, v, _ = fs.export_bsr()
    n = fs.n_nodes
    K = dynamics.to_matrix((r, c, v))
    Kabs = abs(K)
    n_i = np.repeat(6.0 * np.diff(r), 6)
    free = free_of(dmask, n)
    X = np.random.default_rng(5).normal(size=(8, 6 * n)) * free
    want = (K @ X.T).T
    bound = 2.0 * n_i * EPS * (Kabs @ np.abs(X).T).T
    y = fs.spmv(X[0])
    assert (np.abs(y - want[0]) <= bound[0]).all()
    worst = 0.0
    for nc in (1, 3, 4, 5, 8):
        Y = fs.spmm(X[:nc])
        assert Y.shape == (nc, 6 * n)
        err = np.abs(Y - want[:nc])
        worst = max(worst, (err / np.maximum(bound[:nc], 1e-300)).max())
        assert (err <= bound[:nc]).all(), (name, nc)
        # columns that are zero on the constrained dofs stay zero there
        assert (Y[:, ~free] == 0.0).all()
    print("spmm %s: worst error %.3f of the bound" % (name, worst))
    if name == "full":
        fs.set_density(RHO)
        info = fs.modes(2, max_it=2, want_modes=False)[3]
        assert info["fused_product"] == 0
    elif name == "curved":
        info = fs.modes(2, max_it=2, want_modes=False)[3]
        assert info["fused_product"] == 1
    fs.close()


# ------------------------------------------------------------------ 2. Gram matrices

@pytest.mark.parametrize("mesh", ["patch", "one_slice_and_a_node"])
def test_gram_meets_the_dot_product_bound_and_is_reproducible(mesh):
    m = sections.curved_patch(24, 18) if mesh == "patch" else meshes.structured(10, 2, 0, 0, 1, 1, "t")
    assert m.n_nodes == (475 if mesh == "patch" else 33)
    fs = context(m, bc=False)
    mass = dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T).ravel()
    n = 6 * m.n_nodes
    rng = np.random.default_rng(9)
    for qa, qb in ((1, 1), (5, 3), (24, 24), (96, 96)):
        A, B = rng.normal(size=(qa, n)), rng.normal(size=(qb, n))
        for weighted in (True, False):
            w = mass if weighted else np.ones(n)
            G = fs.modal_gram(A, B, weighted)
            want = (A * w) @ B.T
            bound = 2.0 * n * EPS * ((np.abs(A) * w) @ np.abs(B).T)
            assert G.shape == (qa, qb) and (np.abs(G - want) <= bound).all(), (qa, qb, weighted)
            np.testing.assert_array_equal(G, fs.modal_gram(A, B, weighted))
    fs.close()


# ------------------------------------------------------------------ 3. modes against the dense reference

def check_modes(fs, m, mass, shift=0.0, max_it=360, label=""):
    """the assertions of the issue's test 3 on one context; returns (lam, modes, info)"""
    dmask = m.dirichlet_mask()
    fs.assemble()
    r, c, v, _ = fs.export_bsr()
    K = dynamics.to_matrix((r, c, v))
    lam_ref, X_ref = modal.reference(K, mass, dmask, N_MODES + 4, shift)
    lam, modes, res, info = fs.modes(N_MODES, tol=TOL, shift=shift, max_it=max_it)
    print("modes %s: %d iterations, %d restarts, block %d, worst residual %.2e, worst lambda deviation %.2e" % (
        label, info["iterations"], info["restarts"], info["block"], info["residual_max"],
        (np.abs(lam - lam_ref[:N_MODES]) / (lam_ref[:N_MODES] + shift)).max()))
    assert info["converged"] == N_MODES and info["iterations"] <= max_it and info["block"] == N_MODES + 4
    assert (np.diff(lam) >= 0.0).all()
    assert (np.abs(lam - lam_ref[:N_MODES]) <= 1e-8 * (lam_ref[:N_MODES] + shift)).all()
    groups = modal.clusters(lam_ref, shift)
    X = modes.reshape(N_MODES, -1)
    for j in range(N_MODES):
        d = modal.subspace_distance(X[j], X_ref[modal.cluster_of(j, groups)], mass)
        assert d <= 1e-3, (j, d)
    mw = np.asarray(mass).ravel()
    assert np.abs((X * mw) @ X.T - np.eye(N_MODES)).max() <= 1e-10
    assert (X[:, ~free_of(dmask, m.n_nodes)] == 0.0).all()
    rn = modal.residual_norms(K, mass, dmask, lam, X, shift)
    assert (rn <= 2.0 * TOL).all() and (res <= TOL).all() and info["residual_max"] == res.max()
    for j in range(N_MODES):  # the entry of largest magnitude is positive (argmax: the lowest index on ties)
        assert X[j, int(np.argmax(np.abs(X[j])))] > 0.0
    return lam, modes, info


def quad_patch():
    m = meshes.structured(10, 8, 0, 0, 4, 3, kind="q", bcids=(0, -1, 1, -1))
    m.xyz[:, 2] = 0.3 * np.sin(1.3 * m.xyz[:, 0]) * np.cos(0.7 * m.xyz[:, 1])
    return m


def test_modes_of_the_curved_patch_with_multigrid():
    m = sections.curved_patch(24, 18)
    fs = context(m, "amg_small")
    check_modes(fs, m, dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T), max_it=360, label="curved 24 x 18, multigrid")
    assert len(fs.amg_levels()) >= 2
    fs.close()


def test_modes_of_the_small_patch_with_block_jacobi():
    m = sections.curved_patch(12, 10)
    fs = context(m, "jacobi")
    check_modes(fs, m, dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T), max_it=3000, label="curved 12 x 10, block-Jacobi")
    fs.close()


def test_modes_of_the_quadrilateral_patch():
    m = quad_patch()
    fs = context(m, "amg")
    check_modes(fs, m, dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T), label="quadrilaterals 10 x 8")
    fs.close()


def test_modes_of_three_strips_with_a_density_per_section():
    cs = sections.three_strips()
    fs = cs.apply(pkg.FemShell(NU, E, T), loads=False)
    fs.set_density(0.0, section_rho=SECTION_RHO)
    set_pc(fs, "amg_small")
    mass = dynamics.lumped_mass(cs.xyz, cs.tri, cs.quad, SECTION_RHO, cs.sections[:, 2], cs.tri_section, cs.quad_section)
    check_modes(fs, Mesh(cs.xyz, cs.tri, cs.quad, cs.dmask), mass, label="three strips")
    fs.close()


def test_modes_of_the_square_plate_with_its_degenerate_pair():
    m = meshes.structured(16, 16, 0, 0, 1, 1, "t", bcids=(0, 0, 0, 0))
    fs = context(m, "amg_small")
    mass = dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T)
    lam, _, _ = check_modes(fs, m, mass, label="square plate 16 x 16")
    assert abs(lam[2] - lam[1]) <= 1e-2 * lam[2]  # modes 2 and 3: one cluster
    assert abs(lam[0] - modal.plate_first_eigenvalue(E, NU, T, RHO)) <= 0.01 * lam[0]
    fs.close()


def test_modes_keep_the_callers_numbering_under_morton_reordering(monkeypatch):
    m = sections.curved_patch(24, 18)
    mass = dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T)
    plain = context(m, "amg_small")
    lam0 = plain.modes(N_MODES, tol=TOL, max_it=360, want_modes=False)[0]
    plain.close()
    monkeypatch.setenv("FEMSHELL_REORDER", "morton")
    fs = context(m, "amg_small")
    lam, _, _ = check_modes(fs, m, mass, label="curved 24 x 18, Morton order")  # (shapes against the reference in the caller's numbering)
    assert (np.abs(lam - lam0) <= 2e-8 * lam0).all()
    fs.close()


# ------------------------------------------------------------------ 4. free-free

def test_free_free_patch_needs_a_shift():
    m = sections.curved_patch(12, 10)
    free_mesh = Mesh(m.xyz, m.tri, m.quad, None)
    mass = dynamics.lumped_mass(m.xyz, m.tri, m.quad, RHO, T)
    shift = 1e3
    fs = context(m, "amg", bc=False)
    fs.assemble()
    K = dynamics.to_matrix(fs.export_bsr()[:3])
    lam_ref, _ = modal.reference(K, mass, None, N_MODES + 4, shift)
    # the reference itself: three rigid translations, then the values of the CPU restatement
    assert (np.abs(lam_ref[:3]) <= 1e-8 * shift).all()
    listed = np.array([459.8, 497.4, 2226.9, 8433.0, 24909.0])
    assert (np.abs(lam_ref[3:8] - listed) <= 2e-4 * listed).all(), lam_ref[:8]
    assert modal.clusters(lam_ref, shift)[0] == [0, 1, 2]
    check_modes(fs, free_mesh, mass, shift=shift, label="free-free 12 x 10, shift 1e3")
    # without a shift K is singular: the call returns -- an error code from the host's checks, or pairs -- and the context stays usable
    set_pc(fs, "jacobi")
    try:
        lam, _, _, info = fs.modes(N_MODES, tol=TOL, shift=0.0, max_it=40)
        assert info["iterations"] <= 40 and np.isfinite(lam).all()
    except pkg.FemShellError as e:
        assert e.code == BREAKDOWN and "shift" in str(e)
    set_pc(fs, "amg")
    check_modes(fs, free_mesh, mass, shift=shift, label="free-free again")
    fs.close()


# ------------------------------------------------------------------ 5. reproducibility and lifecycle

def refused(call, *args, **kwargs):
    with pytest.raises(pkg.FemShellError) as e:
        call(*args, **kwargs)
    assert e.value.code == INVALID, e.value
    return str(e.value)


def test_two_runs_give_the_same_bits():
    m = sections.curved_patch(12, 10)
    fs = context(m, "amg_small")
    a = fs.modes(N_MODES, tol=TOL, max_it=360)
    b = fs.modes(N_MODES, tol=TOL, max_it=360)
    other = context(m, "amg_small")
    c = other.modes(N_MODES, tol=TOL, max_it=360)
    for x in (b, c):
        np.testing.assert_array_equal(a[0], x[0])
        np.testing.assert_array_equal(a[1], x[1])
        np.testing.assert_array_equal(a[2], x[2])
        assert a[3]["iterations"] == x[3]["iterations"]
    assert a[3]["converged"] == N_MODES
    fs.close()
    other.close()


def test_refusals_leave_the_context_as_it_was():
    m = sections.curved_patch(12, 10)
    empty = pkg.FemShell(NU, E, T)
    refused(empty.modes, 4)  # no mesh
    empty.close()
    fs = context(m, "jacobi", density=None)
    fs.set_loads(m.loads)
    fs.assemble()
    before = fs.export_bsr()
    refused(fs.modes, 4)  # no density
    fs.set_density(RHO)
    refused(fs.modes, 0)
    refused(fs.modes, -3)
    refused(fs.modes, 29)            # 29 + 4 > 32
    refused(fs.modes, 8, guard=25)
    refused(fs.modes, 8, guard=-1)
    refused(fs.modes, 4, tol=0.0)
    refused(fs.modes, 4, tol=-1e-6)
    refused(fs.modes, 4, tol=np.nan)
    refused(fs.modes, 4, shift=-1.0)
    refused(fs.modes, 4, max_it=0)
    fs.dynamics_begin(1e-3)
    refused(fs.modes, 4)             # dynamics is active
    fs.dynamics_end()
    fs.assemble()  # (dynamics_end marks K for re-assembly)
    for x, y in zip(before, fs.export_bsr()):
        np.testing.assert_array_equal(x, y)
    # fewer than 3 (n_modes + guard) free dofs: two triangles, one node free
    tiny = meshes.structured(1, 1, 0, 0, 1, 1, "t")
    small = pkg.FemShell(NU, E, T)
    small.set_mesh(tiny.xyz, tiny.tri, tiny.quad)
    mask = np.full(tiny.n_nodes, 0x3F, np.uint8)
    mask[0] = 0
    small.set_dirichlet(mask)
    small.set_density(RHO)
    refused(small.modes, 1, guard=2)  # 6 free dofs < 9
    small.close()
    # modes after dynamics_end works and is what a context that never stepped gives
    lam, modes, _, info = fs.modes(4, tol=TOL, max_it=3000)
    fresh = context(m, "jacobi")
    lam2, modes2, _, _ = fresh.modes(4, tol=TOL, max_it=3000)
    assert info["converged"] == 4
    np.testing.assert_array_equal(lam, lam2)
    np.testing.assert_array_equal(modes, modes2)
    fs.close()
    fresh.close()


def test_after_a_shifted_run_the_context_is_what_a_fresh_one_is():
    m = sections.curved_patch(12, 10)
    fs = context(m, "amg_small")
    fs.set_loads(m.loads)
    _, _, _, info = fs.modes(4, tol=TOL, shift=50.0, max_it=360)
    assert info["converged"] == 4
    fresh = context(m, "amg_small")
    fresh.set_loads(m.loads)
    fs.assemble()
    fresh.assemble()
    for x, y in zip(fs.export_bsr(), fresh.export_bsr()):
        np.testing.assert_array_equal(x, y)
    u, i1 = fs.solve(rtol=1e-12, max_it=5000)
    u2, i2 = fresh.solve(rtol=1e-12, max_it=5000)
    assert i1["converged"] == 1 and i1["iterations"] == i2["iterations"]
    np.testing.assert_array_equal(u, u2)
    fs.close()
    fresh.close()


# ------------------------------------------------------------------ 6. the host program

HOST = os.path.join(ROOT, "fem-shell_amd", "host")


def _point_vectors(vtk_path, name, n_nodes):
    lines = open(vtk_path).read().splitlines()
    at = lines.index("VECTORS %s double" % name)
    return np.array([[float(t) for t in l.split()] for l in lines[at + 1:at + 1 + n_nodes]])


def test_fem_shell_writes_the_modes_the_binding_gives(tmp_path):
    """FEM-shell -rho -modes: the same library, the same calls (multigrid by default, guard 4, 500 iterations)"""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    m = meshes.load_example("test_E_uvw_t")
    rho = 2.5e-4
    out = str(tmp_path / "E")
    r = subprocess.run([os.path.join(HOST, "FEM-shell"), "-nu", "0.3", "-e", "1e4", "-t", "0.25", "-mesh",
                        os.path.join(meshes.MESH_DIR, "test_E_uvw_t.xda"), "-out", out, "-rho", repr(rho), "-modes", "4"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = np.loadtxt(out + "_modes.txt")
    assert got.shape == (4, 4) and list(got[:, 0]) == [1, 2, 3, 4]
    fs = pkg.FemShell(0.3, 1e4, 0.25)
    fs.set_mesh(m.xyz, m.tri, m.quad)
    fs.set_dirichlet(m.dirichlet_mask())
    fs.set_loads(m.loads)
    fs.set_preconditioner("amg")
    fs.set_density(rho)
    lam, modes, res, info = fs.modes(4)
    fs.close()
    assert info["converged"] == 4
    # '%.15e': sixteen significant digits
    assert (np.abs(got[:, 1] - lam) <= 1e-15 * np.abs(lam)).all()
    assert (np.abs(got[:, 2] - np.sqrt(lam) / (2.0 * np.pi)) <= 4e-15 * got[:, 2]).all()
    assert (np.abs(got[:, 3] - res) <= 1e-15 * np.abs(res)).all()
    for k in range(4):
        np.testing.assert_array_equal(_point_vectors(out + ".vtk", "mode_%d_u" % (k + 1), m.n_nodes), modes[k][:, :3])
        np.testing.assert_array_equal(_point_vectors(out + ".vtk", "mode_%d_r" % (k + 1), m.n_nodes), modes[k][:, 3:])
