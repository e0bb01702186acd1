"""Assembly, products, mass and one solve at the limits of the plan's encodings ("Limits of the plan's encodings";
the plan's side of them is pinned on the CPU by tests/test_plan_limits_cpu.py): block slots of up to 300 contributions, a
constrained node with more than 255 elements, more than 64 KiB of assembly LDS, a slice whose in-slice products exceed the 255
positions of LDS, full-storage rows of 42, 43 and 64 blocks, and the refusals beyond.

Bounds.  K against the oracle: 1e-12, the project's figure, here per stored block, max|K_b - K_b^oracle| <= 1e-12 max|K_b^oracle|
(two summation orders of the oracle itself -- the element list reversed -- differ block by block by at most 1.2e-15 on coil(300)
and 4.3e-16 on clique(32)).  Two kernels: 1e-13 of the block maximum (tests/test_gpu_parity.py).  Diagonal entries of constrained
dofs -- element counts, small integers -- and F: exact.  Products: the dot-product bound of tests/test_gpu_modal.py,
|err_i| <= 2 n_i eps (|K||x|)_i with n_i = 6 x blocks in row i; residual: 1e-11 ||F|| against the longdouble residual
(tests/test_gpu_amg.py); mass: 1e-13 per entry (tests/test_gpu_dynamics.py)."""
import functools

import numpy as np
import pytest

from oracle import amg_oracle
from tests.helpers import dynamics, meshes, oracle, sections
from tests.helpers.product import ensure_built

pytestmark = pytest.mark.gpu
pkg = ensure_built()

NU, E, T, RHO = 0.3, 2.1e5, 0.04, 7.8e-3
EPS = np.finfo(np.float64).eps
UNSUPPORTED = -7
NO_TRIS, NO_QUADS = np.zeros((0, 3), np.int32), np.zeros((0, 4), np.int32)


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    """(xyz, tri, quad, hub or None) of "coil300", "quad_petals258", "mixed_petals150", "clique32" (with its strips)"""
    kind, size = name.rstrip("0123456789"), int(name[len(name.rstrip("0123456789")):])
    if kind == "coil":
        xyz, tri = meshes.coil(size)
        return xyz, tri, NO_QUADS, len(xyz) - 1
    if kind == "quad_petals":
        xyz, quad = meshes.quad_petals(size)
        return xyz, NO_TRIS, quad, len(xyz) - 1
    if kind == "mixed_petals":
        xyz, tri, quad = meshes.mixed_petals(size)
        return xyz, tri, quad, len(xyz) - 1
    xyz, tri = meshes.clique(size)
    return xyz, tri, NO_QUADS, None


def constraints_and_loads(n, hub, hub_mask):
    """the hub's mask, a mask drawn from a fixed generator on every seventh other node, random loads"""
    rng = np.random.default_rng(12)
    others = np.array([a for a in range(n) if a != hub])[::7]
    dmask = np.zeros(n, np.uint8)
    dmask[others] = rng.integers(1, 64, len(others)).astype(np.uint8)
    if hub is not None:
        dmask[hub] = hub_mask
    return dmask, rng.normal(size=(n, 6))


@functools.lru_cache(maxsize=None)
def case_of(name, hub_mask):
    """(xyz, tri, quad, dmask, loads, the oracle's (rowptr, colidx, vals, F)): computed once, shared, never written to"""
    xyz, tri, quad, hub = mesh_of(name)
    dmask, loads = constraints_and_loads(len(xyz), hub, hub_mask)
    ref = oracle.assemble(xyz, tri, quad, oracle.material(NU, E, T), dmask, loads)
    return xyz, tri, quad, dmask, loads, ref


def worst_block_ratio(v, v0):
    """max over the stored blocks of max|K_b - K_b^ref| / max|K_b^ref|; a block that is zero in the reference must be zero"""
    d, s = np.abs(v - v0).max(axis=(1, 2)), np.abs(v0).max(axis=(1, 2))
    assert np.all(d[s == 0.0] == 0.0)
    return float((d[s > 0.0] / s[s > 0.0]).max())


def constrained_diagonal(rowptr, colidx, vals, dmask):
    """the diagonal entries of the constrained dofs, node by node"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    diag = np.flatnonzero(colidx == rows)
    assert len(diag) == len(rowptr) - 1
    fixed = ~dynamics.free_dofs(dmask, len(dmask)).reshape(-1, 6)
    return vals[diag][:, np.arange(6), np.arange(6)][fixed]


def assembled(monkeypatch, xyz, tri, quad, dmask, loads, pipe, prepare=None):
    """K and F through the two-phase kernel (pipe "0") or the pipelined one ("2"), assembled twice: the same bits"""
    monkeypatch.setenv("FEMSHELL_ASM_PIPE", pipe)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    if prepare is not None:
        prepare(fs)
    assert fs.assembly_kernel() == ("k_assemble_pipe" if pipe == "2" else "k_assemble")
    fs.assemble()
    out = fs.export_bsr()
    fs.assemble()
    again = fs.export_bsr()
    fs.close()
    np.testing.assert_array_equal(again[2], out[2])
    np.testing.assert_array_equal(again[3], out[3])
    return out


# ------------------------------------------------------------------ a. K and F against the oracle, block by block

HUBS = ["coil85", "coil86", "coil128", "coil129", "coil255", "coil256", "coil300", "quad_petals86", "quad_petals258",
        "mixed_petals150"]
ASSEMBLY_CASES = ([(name, mask, "1") for name in HUBS for mask in (0, 0x3F, 0x15)] +
                  [(name, 0, sym) for name in ("clique24", "clique32") for sym in ("1", "0")] +
                  [(name, mask, "0") for name in ("coil41", "coil62") for mask in (0, 0x3F, 0x15)])  # rows of 43 and 64 blocks


@pytest.mark.parametrize("name,hub_mask,symmetric", ASSEMBLY_CASES)
def test_assembled_matrix_equals_the_oracle_block_by_block(monkeypatch, name, hub_mask, symmetric):
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", symmetric)
    xyz, tri, quad, dmask, loads, (r0, c0, v0, F0) = case_of(name, hub_mask)
    monkeypatch.setenv("FEMSHELL_ASM_PIPE", "2")  # 2: the pipelined layout wherever the kernel can run
    pipes = ["0", "2"] if pkg.build_plan(xyz, tri, quad)["pipe"] == 1 else ["0"]
    if name in ("coil85", "coil86", "coil128") and symmetric == "1":
        assert pipes == ["0", "2"]
    if name in ("coil129", "coil300", "quad_petals86"):
        assert pipes == ["0"]
    hub = mesh_of(name)[3]
    out = {}
    for pipe in pipes:
        r, c, v, F = out[pipe] = assembled(monkeypatch, xyz, tri, quad, dmask, loads, pipe)
        np.testing.assert_array_equal(r, r0)
        np.testing.assert_array_equal(c, c0)
        np.testing.assert_array_equal(F, F0)
        worst = worst_block_ratio(v, v0)
        print("%s hub mask %#x symmetric %s pipe %s: worst block %.2e" % (name, hub_mask, symmetric, pipe, worst))
        assert worst <= 1e-12
        got, want = constrained_diagonal(r, c, v, dmask), constrained_diagonal(r0, c0, v0, dmask)
        np.testing.assert_array_equal(got, want)
        if hub is not None and hub_mask:  # one per element at the hub
            n_elems = int(np.count_nonzero(tri == hub) + np.count_nonzero(quad == hub))
            size = int(name.lstrip("abcdefghijklmnopqrstuvwxyz_"))
            assert n_elems == (3 * size // 2 if name.startswith("mixed") else size)
            for i in range(6):
                if (hub_mask >> i) & 1:
                    assert v[r[hub + 1] - 1, i, i] == float(n_elems)  # (the hub is numbered last: its diagonal block too)
    if len(pipes) == 2:
        both = worst_block_ratio(out["2"][2], out["0"][2])
        print("%s: the two kernels differ by %.2e of a block" % (name, both))
        assert both <= 1e-13


# ------------------------------------------------------------------ b. sections on a deep slot

def test_sections_on_a_slot_of_300_contributions(monkeypatch):
    """coil(300), three sections by k % 3 (thickness 0.02 / 0.04 / 0.08, Young's moduli 1 : 3 : 9), the hub clamped: against the
    oracle's assembly section by section, summed, as tests/test_gpu_sections.py does -- with the bound per block"""
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    xyz, tri, quad, hub = mesh_of("coil300")
    dmask = np.zeros(len(xyz), np.uint8)
    dmask[hub] = 0x3F
    loads = np.random.default_rng(3).normal(size=(len(xyz), 6))
    sec = np.array([[0.3, 7.0e4, 0.02], [0.3, 2.1e5, 0.04], [0.3, 6.3e5, 0.08]])
    cs = sections.Case(xyz, tri, None, sec, np.arange(len(tri), dtype=np.int32) % 3, None, dmask, loads)
    r0, c0, v0, F0 = sections.reference(cs)
    r, c, v, F = assembled(monkeypatch, xyz, tri, quad, dmask, loads, "0",
                           prepare=lambda fs: fs.set_sections(cs.sections, cs.tri_section))
    np.testing.assert_array_equal(r, r0)
    np.testing.assert_array_equal(c, c0)
    np.testing.assert_array_equal(F, F0)
    worst = worst_block_ratio(v, v0)
    print("coil300 with three sections: worst block %.2e" % worst)
    assert worst <= 1e-12
    np.testing.assert_array_equal(constrained_diagonal(r, c, v, dmask), constrained_diagonal(r0, c0, v0, dmask))
    assert np.all(np.diag(v[r[hub + 1] - 1]) == 300.0)


# ------------------------------------------------------------------ c. products through a hub and through a full slice

PRODUCT_CASES = [("coil300", 0, "1"), ("coil300", 0x3F, "1"), ("clique19", 0, "1"), ("clique23", 0, "1"), ("clique32", 0, "1"),
                 ("coil40", 0, "0"), ("coil41", 0, "0"), ("coil62", 0, "0")]


def product_context(monkeypatch, name, hub_mask, symmetric, local=None):
    monkeypatch.setenv("FEMSHELL_SYMMETRIC", symmetric)
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    if local is None:
        monkeypatch.delenv("FEMSHELL_SPMV_LOCAL", raising=False)
    else:
        monkeypatch.setenv("FEMSHELL_SPMV_LOCAL", local)
    xyz, tri, quad, hub = mesh_of(name)
    dmask, loads = constraints_and_loads(len(xyz), hub, hub_mask)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.assemble()
    return fs, dmask


@pytest.mark.parametrize("name,hub_mask,symmetric", PRODUCT_CASES)
def test_products_meet_the_dot_product_bound(monkeypatch, name, hub_mask, symmetric):
    """spmv, spmm with 1, 3, 4, 5 and 8 columns and the double-double residual.  coil(300): the hub's row has 302 blocks and
    its in-list 301 entries; clique(19) / (23) / (32): 171, 253 and 276 in-slice products of one slice (two columns per pass of
    the block product above 170, 21 products beyond the 255 positions of LDS), the clique in the second half of its workgroup;
    full storage: rows of 42, 43 and 64 blocks -- under 64 KiB of x in LDS, over it, the widest a context accepts."""
    fs, dmask = product_context(monkeypatch, name, hub_mask, symmetric)
    r, c, v, F = fs.export_bsr()
    n = fs.n_nodes
    if name == "coil300":
        assert np.diff(r).max() == 302
    if symmetric == "0":
        assert np.diff(r).max() == int(name[4:]) + 2
    K = dynamics.to_matrix((r, c, v))
    Kabs = abs(K)
    n_i = np.repeat(6.0 * np.diff(r), 6)
    free = dynamics.free_dofs(dmask, n)
    X = np.random.default_rng(5).normal(size=(8, 6 * n)) * free
    K.sort_indices()
    data, starts = K.data.astype(np.longdouble), K.indptr[:-1]
    assert np.all(np.diff(K.indptr) > 0)
    want = np.stack([np.add.reduceat(data * x.astype(np.longdouble)[K.indices], starts) for x in X])
    bound = 2.0 * n_i * EPS * (Kabs @ np.abs(X).T).T
    y = fs.spmv(X[0])
    assert (np.abs(y - want[0]) <= bound[0]).all()
    assert (y[~free] == 0.0).all()
    worst = float((np.abs(y - want[0]) / np.maximum(bound[0], 1e-300)).max())
    for nc in (1, 3, 4, 5, 8):
        Y = fs.spmm(X[:nc])
        assert Y.shape == (nc, 6 * n)
        err = np.abs(Y - want[:nc]).astype(np.float64)
        worst = max(worst, float((err / np.maximum(bound[:nc], 1e-300)).max()))
        assert (err <= bound[:nc]).all(), (name, nc)
        assert (Y[:, ~free] == 0.0).all()  # columns that are zero on the constrained dofs stay zero there
    print("products %s hub mask %#x: worst error %.3f of the bound" % (name, hub_mask, worst))
    # the residual F - K x of an x for which K x is of the size of F (its result is rounded to FP64 once, relative to itself)
    nb = np.linalg.norm(F)
    x = X[0] * (nb / np.linalg.norm(K @ X[0]))
    r_dd, r_ext = fs.residual(x), amg_oracle.residual_extended(K, F, x)
    print("residual %s: deviation %.2e ||F||" % (name, np.linalg.norm(r_dd - r_ext) / nb))
    assert np.linalg.norm(r_dd - r_ext) <= 1e-11 * nb
    fs.close()


def test_spilled_in_slice_products_equal_the_products_through_hbm(monkeypatch):
    """clique(32): FEMSHELL_SPMV_LOCAL=0 sends every transposed product through HBM -- the same product to the tolerance of
    test_products_kept_in_the_slice_equal_the_products_through_hbm (which does not ask for the same bits: the sums of a row
    take another order), each reproducible bit by bit"""
    x = None
    ys = {}
    for local in ("1", "0"):
        fs, dmask = product_context(monkeypatch, "clique32", 0, "1", local=local)
        if x is None:
            x = np.random.default_rng(2).normal(size=6 * fs.n_nodes)
        y1, y2 = fs.spmv(x), fs.spmv(x)
        np.testing.assert_array_equal(y1, y2)
        r, c, v, _ = fs.export_bsr()
        ys[local] = y1
        fs.close()
    y0 = oracle.spmv(r, c, v, x)
    scale = np.abs(v).max() * np.abs(x).max()
    print("clique32: in the slice %.2e, through HBM %.2e of the scale; same bits: %s"
          % (np.abs(ys["1"] - y0).max() / scale, np.abs(ys["0"] - y0).max() / scale, np.array_equal(ys["1"], ys["0"])))
    assert np.abs(ys["1"] - y0).max() <= 1e-13 * scale and np.abs(ys["0"] - y0).max() <= 1e-13 * scale


# ------------------------------------------------------------------ d. mass, shift and one solve

@pytest.mark.parametrize("name", ["coil300", "quad_petals258"])
def test_lumped_mass_of_a_hub(monkeypatch, name):
    """the hub sums 300 (258) shares"""
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    xyz, tri, quad, hub = mesh_of(name)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri, quad)
    fs.set_density(RHO)
    got, want = fs.lumped_mass(), dynamics.lumped_mass(xyz, tri, quad, RHO, T)
    fs.close()
    assert got.shape == want.shape and (want > 0.0).all()
    worst = (np.abs(got - want) / want).max()
    print("lumped mass %s: worst relative deviation per entry %.2e, at the hub %.2e" % (name, worst, (np.abs(got - want) / want)[hub].max()))
    assert worst <= 1e-13


def test_dynamics_begin_and_end_give_k_back_bitwise(monkeypatch):
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    xyz, tri, quad, dmask, loads, _ = case_of("coil300", 0x15)
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.set_density(RHO)
    fs.assemble()
    r0, c0, v0, F0 = fs.export_bsr()
    fs.dynamics_begin(1e-3, beta=0.3025, gamma=0.6, alpha=3.0)
    _, _, v1, _ = fs.export_bsr()
    hub = len(xyz) - 1
    d0, d1 = np.diag(v0[r0[hub + 1] - 1]), np.diag(v1[r0[hub + 1] - 1])
    assert np.all((d1 > d0) == ((0x15 >> np.arange(6)) & 1 == 0))  # shifted on the hub's free dofs, the counts untouched
    fs.dynamics_end()
    fs.assemble()
    _, _, v2, F2 = fs.export_bsr()
    fs.close()
    np.testing.assert_array_equal(v2, v0)
    np.testing.assert_array_equal(F2, F0)


def true_relative_residual(K, F, u):
    return float(np.linalg.norm(amg_oracle.residual_extended(K, F, u)) / np.linalg.norm(F))


def test_one_block_jacobi_solve_through_the_hub(monkeypatch):
    """coil(300), the hub free, every fifth ring node clamped, unit load in z, rtol 1e-10: converged, and the true relative
    residual (longdouble, on the exported matrix) no more than ten times that of the oracle's block-Jacobi CG on the same
    matrix at the same rtol -- the factor is there for two correct recurrences that round differently."""
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    xyz, tri, quad, hub = mesh_of("coil300")
    dmask = np.zeros(len(xyz), np.uint8)
    dmask[0:hub:5] = 0x3F
    loads = np.zeros((len(xyz), 6))
    loads[:, 2] = 1.0
    fs = pkg.FemShell(NU, E, T)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    u, info = fs.solve(rtol=1e-10, max_it=20000)
    r, c, v, F = fs.export_bsr()
    fs.close()
    assert info["converged"] == 1, info
    K = dynamics.to_matrix((r, c, v))
    u0, info0 = oracle.pcg(r, c, v, F, rtol=1e-10, max_it=20000)
    assert info0["converged"] == 1, info0
    res, res0 = true_relative_residual(K, F, u.ravel()), true_relative_residual(K, F, u0)
    print("coil300 solve: device %d iterations, true relative residual %.3e; oracle %d iterations, %.3e"
          % (info["iterations"], res, info0["iterations"], res0))
    assert res <= 10.0 * res0


# ------------------------------------------------------------------ e. refusals

@pytest.mark.parametrize("case", ["lds_staging", "neighbours", "contributions"])
def test_refused_meshes_leave_the_context_usable(monkeypatch, case):
    """765 elements at a node exceed the assembly kernel's LDS, 64 neighbours in full storage the widest slice, 766
    contributions the plan's chunk count: FEMSHELL_ERR_UNSUPPORTED each, and the same context then takes coil(85) and assembles
    the bits a fresh context gives."""
    monkeypatch.delenv("FEMSHELL_ASM_PIPE", raising=False)
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    v, message = {"lds_staging": (765, "too many elements for the LDS staging"), "neighbours": (63, "more than 63 neighbours"),
                  "contributions": (766, "more than 765 contributions")}[case]
    xyz, tri, quad, dmask, loads, _ = case_of("coil85", 0x15)
    fresh = pkg.FemShell(NU, E, T)
    fresh.set_mesh(xyz, tri, quad)
    fresh.set_dirichlet(dmask)
    fresh.set_loads(loads)
    fresh.assemble()
    want = fresh.export_bsr()
    fresh.close()
    fs = pkg.FemShell(NU, E, T)
    if case == "neighbours":
        monkeypatch.setenv("FEMSHELL_SYMMETRIC", "0")
    with pytest.raises(pkg.FemShellError) as ei:
        fs.set_mesh(*meshes.coil(v))
    assert ei.value.code == UNSUPPORTED and message in str(ei.value)
    monkeypatch.delenv("FEMSHELL_SYMMETRIC", raising=False)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.assemble()
    got = fs.export_bsr()
    fs.close()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
