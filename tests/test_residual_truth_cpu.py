"""The truth, the budget and the model of tests/helpers/residual_truth.py, on the CPU: what tests/test_gpu_residual_truth.py holds
k_residual_dd and k_residual_dd_sym to is pinned here without a device.

  * exact() equals rational arithmetic on a handful of rows;
  * the restatement of the kernels' arithmetic meets the budget on every row in every state, in both orders of the terms -- the
    derivation of the budget (Dot2, Prop. 5.5 of Ogita, Rump and Oishi) holds for the algorithm the kernels implement;
  * four planted defects -- the ways a double-double residual turns into an FP64 one without anything failing -- each exceed
    the budget on at least one row of the cancelling state;
  * the gap this closes: on the non-cancelling input of tests/test_gpu_limits.py a plain FP64 residual passes the older
    assertion, 1e-11 ||F|| against amg_oracle.residual_extended, and fails the budget;
  * residual_extended itself, 64 bits of significand, against the truth where seven digits cancel: why it is not the reference
    here.

Matrices: the oracle's assembly of sections.curved_patch(12, 10) (143 nodes, rows of up to 7 blocks, a clamped and a simply
supported edge) and of meshes.coil(40) (42 nodes, a hub row of 42 blocks, m = 254, every seventh node with a random mask)."""
import functools

import numpy as np
import pytest

from oracle import amg_oracle
from tests.helpers import dynamics, meshes, oracle, sections
from tests.helpers import residual_truth as rt

NU, E, T = 0.3, 2.1e5, 0.04
ALL_STATES = rt.STATES + ("iterate",)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(K, {state: (x, F)}): computed once, shared, never written to"""
    if name == "patch":
        m = sections.curved_patch(12, 10)
        xyz, tri, quad, dmask, loads = m.xyz, m.tri, m.quad, m.dirichlet_mask(), m.loads
    else:
        xyz, tri = meshes.coil(40)
        quad = np.zeros((0, 4), np.int32)
        rng = np.random.default_rng(12)
        dmask = np.zeros(len(xyz), np.uint8)
        dmask[::7] = rng.integers(1, 64, len(dmask[::7])).astype(np.uint8)
        loads = rng.normal(size=(len(xyz), 6))
    r, c, v, F = oracle.assemble(xyz, tri, quad, oracle.material(NU, E, T), dmask, loads)
    K = (r, c, v)
    st = rt.states(K, F, dynamics.free_dofs(dmask, len(xyz)))
    st["iterate"] = (oracle.direct_solve(r, c, v, F), F)  # a solution to FP64: the state a refinement pass sees
    return K, st


@functools.lru_cache(maxsize=None)
def truth_of(name, state):
    K, st = fixture(name)
    x, F = st[state]
    truth = rt.exact(K, F, x)
    return truth, rt.bound(K, F, x, truth)


def test_split_products_and_the_budget_on_known_numbers():
    a, b = np.array([1.0 + 2.0 ** -30, 3.0, 0.0, -(2.0 ** 400)]), np.array([1.0 + 2.0 ** -30, 1.0 / 3.0, 5.0, 2.0 ** -450 * 1.5])
    p, e = rt.two_product(a, b)
    assert p[0] == 1.0 + 2.0 ** -29 and e[0] == 2.0 ** -60 and p[2] == 0.0 and e[2] == 0.0 and e[3] == 0.0
    assert e[1] == float(3 * rt.Fraction(1.0 / 3.0) - rt.Fraction(float(p[1])))
    with pytest.raises(AssertionError):
        rt.two_product(np.array([2.0 ** 451]), np.array([1.0]))
    with pytest.raises(AssertionError):
        rt.two_product(np.array([1.0]), np.array([2.0 ** -451]))
    # one node, one block: m = 8
    K = (np.array([0, 1]), np.array([0]), np.eye(6)[None])
    g = 8 * rt.U / (1 - 8 * rt.U)
    np.testing.assert_array_equal(rt.bound(K, np.full(6, 3.0), np.ones(6)), rt.U * 2.0 + g * g * 4.0)
    np.testing.assert_array_equal(rt.exact(K, np.full(6, 3.0), np.ones(6)), 2.0)


@pytest.mark.parametrize("name", ["patch", "coil40"])
def test_exact_equals_rational_arithmetic(name):
    K, st = fixture(name)
    n6 = 6 * (len(K[0]) - 1)
    rows = np.unique(np.concatenate([np.random.default_rng(1).integers(0, n6, 8), [0, n6 - 1, n6 - 6]]))  # (the hub's rows too)
    for state in ALL_STATES:
        x, F = st[state]
        np.testing.assert_array_equal(truth_of(name, state)[0][rows], rt.fraction(K, F, x, rows))
    # the cancelling state cancels: the exact residual is the rounding error of the FP64 product, gamma_n (|K||x|)_i at most
    x, F = st["cancel"]
    S = rt.scale(K, F, x)
    assert np.all(np.abs(truth_of(name, "cancel")[0]) <= rt.gamma(6.0 * rt.blocks_per_row(K)) * S)
    assert rt.cancellation(truth_of(name, "cancel")[0], S) < 1e-12
    assert rt.cancellation(truth_of(name, "free")[0], rt.scale(K, *st["free"][::-1])) > 0.1


@pytest.mark.parametrize("order", ["stored", "sym"])
@pytest.mark.parametrize("name", ["patch", "coil40"])
def test_the_model_meets_the_budget_on_every_row_in_every_state(name, order):
    K, st = fixture(name)
    for state in ALL_STATES:
        x, F = st[state]
        truth, budget = truth_of(name, state)
        worst = rt.ratios(rt.model(K, F, x, order=order), truth, budget).max()
        print("model %s %s order %s: worst error %.4f of the budget" % (name, state, order, worst))
        assert worst <= 1.0, (name, state, order, worst)


@pytest.mark.parametrize("defect", rt.DEFECTS)
@pytest.mark.parametrize("name", ["patch", "coil40"])
def test_a_planted_defect_exceeds_the_budget(name, defect):
    K, st = fixture(name)
    for state in ALL_STATES:
        x, F = st[state]
        truth, budget = truth_of(name, state)
        ratio = rt.ratios(rt.model(K, F, x, defect, order="sym"), truth, budget)
        print("defect %s on %s, state %s: worst error %.3g of the budget, %d of %d rows over it"
              % (defect, name, state, ratio.max(), np.count_nonzero(ratio > 1.0), len(ratio)))
        if state in ("cancel", "iterate"):  # (the other two states are reported: little cancels there, a defect costs an ulp or two)
            assert ratio.max() > 1.0, (name, defect, state)
        if state == "cancel" and defect != "contracted":
            assert ratio.max() >= 1e7, (name, defect, state, ratio.max())


@pytest.mark.parametrize("name", ["patch", "coil40"])
def test_a_plain_fp64_residual_passes_the_older_assertion_and_fails_the_budget(name):
    """x scaled so that ||K x|| = ||F|| (tests/test_gpu_limits.py, tests/helpers/grid_worker.py): nothing cancels, and FP64 row
    sums are four digits inside 1e-11 ||F|| -- that assertion does not tell double-double from double on this input"""
    K, st = fixture(name)
    x, F = st["free"]
    r64 = rt.model(K, F, x, "fp64")
    np.testing.assert_array_equal(r64, F - oracle.spmv(*K, x))  # the defect is what it says: the FP64 product, subtracted
    old = np.linalg.norm(r64 - amg_oracle.residual_extended(rt.csr(K), F, x)) / np.linalg.norm(F)
    truth, budget = truth_of(name, "free")
    new = rt.ratios(r64, truth, budget).max()
    print("FP64 row sums on %s, no cancellation: %.2e ||F|| from the long-double residual (allowed 1e-11), %.3g of the budget"
          % (name, old, new))
    assert old <= 1e-11 and new > 1.0
    assert rt.ratios(rt.model(K, F, x), truth, budget).max() <= 1.0


@pytest.mark.parametrize("name", ["patch", "coil40"])
def test_the_long_double_residual_is_no_truth_under_cancellation(name):
    """64 bits against seven digits of cancellation: residual_extended is 1e9 budgets from the truth there (and 1e-19 ||K||x||
    in norm, far inside 1e-11 ||F|| of anything: the older assertions lose nothing by it).  Without cancellation it is the
    truth rounded twice, at most an ulp off."""
    K, st = fixture(name)
    for state in ALL_STATES:
        x, F = st[state]
        truth, budget = truth_of(name, state)
        ext = amg_oracle.residual_extended(rt.csr(K), F, x)
        ratio = rt.ratios(ext, truth, budget).max()
        print("residual_extended on %s, state %s: worst distance from the truth %.3g of the budget, %.2e of ||S||"
              % (name, state, ratio, np.linalg.norm(ext - truth) / np.linalg.norm(rt.scale(K, F, x))))
        if state in ("cancel", "iterate"):
            assert ratio > 1e6
        else:
            assert np.all(np.abs(ext - truth) <= np.spacing(np.abs(truth)))


def test_the_model_meets_the_budget_on_random_rows_over_eight_decades():
    """Not a stiffness matrix: node row a holds the blocks of columns 0..a, 6 to 732 terms a row, entries and x of either sign
    with magnitudes 1e-4 to 1e4, F = fl(K x) (everything cancels) and F random (nothing does), the terms in both orders"""
    n = 122
    rng = np.random.default_rng(21)
    rowptr = np.concatenate([[0], np.cumsum(np.arange(1, n + 1))])
    colidx = np.concatenate([np.arange(a + 1) for a in range(n)])
    vals = rng.choice([-1.0, 1.0], size=(len(colidx), 6, 6)) * 10.0 ** rng.uniform(-4.0, 4.0, size=(len(colidx), 6, 6))
    x = rng.choice([-1.0, 1.0], size=6 * n) * 10.0 ** rng.uniform(-4.0, 4.0, size=6 * n)
    K = (rowptr, colidx, vals)
    assert rt.blocks_per_row(K).min() == 1 and rt.blocks_per_row(K).max() == n
    for state, F in (("cancel", rt.csr(K) @ x), ("random", rng.normal(size=6 * n))):
        truth = rt.exact(K, F, x)
        np.testing.assert_array_equal(truth[::97], rt.fraction(K, F, x, np.arange(0, 6 * n, 97)))
        budget = rt.bound(K, F, x, truth)
        for order in ("stored", "sym"):
            worst = rt.ratios(rt.model(K, F, x, order=order), truth, budget).max()
            print("random rows, %s, order %s: worst error %.4f of the budget" % (state, order, worst))
            assert worst <= 1.0
        assert rt.ratios(rt.model(K, F, x, "fp64"), truth, budget).max() > 1.0
