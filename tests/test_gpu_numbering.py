"""FEMSHELL_REORDER_MORTON / _RCM renumber the nodes inside the library only: the node-indexed entry points that the other
renumbering tests do not reach -- spmm, modal_gram, element_product called directly, set_initial_guess(u0),
dynamics_begin(u0, v0) and dynamics_state -- keep the caller's ids.  A context with the flag against one without, the same
caller-numbered random input to both.

Mesh: meshes.delaunay_patch(600, 2, strips=False), 600 nodes in random caller numbering (600 = 18 * 32 + 24: the last
slice has padding rows), for which neither ordering is the identity; both facts are asserted."""
import functools

import numpy as np
import pytest

from tests.helpers import dynamics, meshes
from tests.helpers.product import ensure_built

pytestmark = pytest.mark.gpu

pkg = ensure_built()

NU, E, T, RHO = 0.3, 7.0e4, 0.03, 7.8e-3
EPS = np.finfo(np.float64).eps
FLAGS = ["REORDER_MORTON", "REORDER_RCM"]


@functools.lru_cache(maxsize=None)
def _mesh():
    xyz, tri = meshes.delaunay_patch(600, 2, strips=False)
    n = len(xyz)
    rng = np.random.default_rng(11)
    dmask = np.zeros(n, np.uint8)
    dmask[xyz[:, 0] < 0.2] = 0x3F
    free = dynamics.free_dofs(dmask, n)
    inputs = dict(loads=rng.normal(size=(n, 6)), X=rng.normal(size=(3, 6 * n)) * free, x=rng.uniform(-1.0, 1.0, 6 * n),
                  A=rng.normal(size=(2, 6 * n)), B=rng.normal(size=(3, 6 * n)), u0=1e-3 * rng.normal(size=6 * n),
                  v0=rng.normal(size=6 * n))
    return xyz, tri, dmask, free, inputs


def _run(flags, guess):
    """every uncovered entry point once on a context with these flags; guess: the start of the last solve (None: the solution
    of an all-but-exact multigrid solve is computed here and returned for the other context)"""
    xyz, tri, dmask, _, inp = _mesh()
    fs = pkg.FemShell(NU, E, T, flags=flags)
    fs.set_mesh(xyz, tri)
    fs.set_dirichlet(dmask)
    fs.set_loads(inp["loads"])
    fs.set_density(RHO)
    fs.assemble()
    out = {"bsr": fs.export_bsr()[:3], "spmm": fs.spmm(inp["X"]), "spmv": np.stack([fs.spmv(col) for col in inp["X"]]),
           "element_product": fs.element_product(inp["x"]), "mass": fs.lumped_mass().ravel()}
    for weighted in (True, False):
        out["gram", weighted] = fs.modal_gram(inp["A"], inp["B"], weighted)
    if guess is None:
        fs.set_preconditioner("amg")
        out["u"], info = fs.solve(rtol=1e-12, max_it=500)
        assert info["converged"] == 1
    else:
        fs.set_initial_guess(guess)
        _, out["warm_info"] = fs.solve(rtol=1e-8, max_it=5000)
    fs.dynamics_begin(1e-3, u0=inp["u0"], v0=inp["v0"])
    out["state"] = fs.dynamics_state()
    fs.dynamics_end()
    fs.close()
    return out


@functools.lru_cache(maxsize=None)
def _plain():
    return _run(pkg.REF_DEFAULT, None)


@functools.lru_cache(maxsize=None)
def _reordered(flag):
    return _run(pkg.REF_DEFAULT | getattr(pkg, flag), _plain()["u"])


def _rel(a, b):
    return np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b))


@pytest.mark.parametrize("kind", ["morton", "rcm"])
def test_the_mesh_is_renumbered_and_has_padding_rows(kind):
    """without these the comparisons below would pass vacuously"""
    xyz, tri = _mesh()[:2]
    perm = pkg.reorder_host(kind, xyz, tri)
    assert not np.array_equal(perm, np.arange(len(xyz)))
    assert len(xyz) % 32 != 0


@pytest.mark.parametrize("flag", FLAGS)
def test_products_keep_the_callers_numbering(flag):
    """spmm and element_product: the same sums in another order, 1e-13 as for spmv in test_gpu_parity.py; the columns of spmm
    against spmv on the reordered context: both meet 2 n_i eps (|K||x|)_i against the exported matrix (test_gpu_modal.py),
    so they differ by twice that at most"""
    p, r = _plain(), _reordered(flag)
    X = _mesh()[4]["X"]
    for what in ("spmm", "element_product"):
        d = _rel(r[what], p[what])
        print("numbering %s %s: relative difference to the plain context %.3e" % (flag, what, d))
        assert d <= 1e-13
    K = dynamics.to_matrix(r["bsr"])
    bound = 2.0 * np.repeat(6.0 * np.diff(r["bsr"][0]), 6) * EPS * (abs(K) @ np.abs(X).T).T
    want = (K @ X.T).T
    assert (np.abs(r["spmm"] - want) <= bound).all() and (np.abs(r["spmv"] - want) <= bound).all()
    assert (np.abs(r["spmm"] - r["spmv"]) <= 2.0 * bound).all()


@pytest.mark.parametrize("flag", FLAGS)
def test_gram_products_keep_the_callers_numbering(flag):
    """A^T diag(w) B with the context's own lumped mass (caller's numbering): the dot-product bound of test_gpu_modal.py"""
    r = _reordered(flag)
    A, B = _mesh()[4]["A"], _mesh()[4]["B"]
    n = A.shape[1]
    for weighted in (True, False):
        w = r["mass"] if weighted else np.ones(n)
        want = (A * w) @ B.T
        bound = 2.0 * n * EPS * ((np.abs(A) * w) @ np.abs(B).T)
        assert r["gram", weighted].shape == (2, 3) and (np.abs(r["gram", weighted] - want) <= bound).all(), weighted


@pytest.mark.parametrize("flag", FLAGS)
def test_initial_guess_is_taken_in_the_callers_numbering(flag):
    """the plain context's solution as the start: converged at once (uploaded in the wrong numbering it takes dozens)"""
    info = _reordered(flag)["warm_info"]
    assert info["converged"] == 1 and info["iterations"] <= 1, info


@pytest.mark.parametrize("flag", FLAGS)
def test_dynamics_state_keeps_the_callers_numbering(flag):
    """u and v straight after dynamics_begin(u0, v0) are copies: bit-equal to the input on the free dofs, the plain context's
    values on the fixed ones.  a = M^-1 (F - K u0) on the free dofs, a product with K and a diagonal solve: it inherits the
    product's reordering noise and nothing else."""
    free, inp = _mesh()[3:]
    (u0, v0, a0), (u1, v1, a1) = _plain()["state"], _reordered(flag)["state"]
    for got, plain, given in ((u1, u0, inp["u0"]), (v1, v0, inp["v0"])):
        np.testing.assert_array_equal(got.ravel()[free], given[free])
        np.testing.assert_array_equal(got.ravel()[~free], plain.ravel()[~free])
    d = _rel(a1, a0)
    print("numbering %s dynamics_state a: relative difference to the plain context %.3e" % (flag, d))
    # measured before the node-vector transfers moved into csrc/node_io.cpp: 1.141e-16 (Morton), 2.604e-16 (RCM); ten times the
    # larger, floored at 1e-13
    assert d <= max(10.0 * 2.604e-16, 1e-13)
