"""CPU pins of tests/helpers/krylov_truth.py, the truth the Krylov loops are held to on the GPU (tests/test_gpu_krylov_truth.py):
exact_dot against rational arithmetic, scalar_phase against hand-computed cases of every phase with every breakdown branch and
the clamps, the restated recurrences against the oracles' histories, reduce_model against exact sums -- and planted defects: the
assertions of the GPU tests, run on a defective model, catch each of them.  No GPU call is made."""
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import krylov_truth as kt
from tests.helpers import oracle, sections

S = kt.Scalars


def test_exact_dot_is_the_correctly_rounded_rational_dot():
    rng = np.random.default_rng(1)
    for n, decades in ((1, 0), (7, 3), (300, 0), (300, 12), (257, 40)):
        a = rng.standard_normal(n) * 10.0 ** rng.uniform(-decades, decades, size=n)
        b = rng.standard_normal(n) * 10.0 ** rng.uniform(-decades, decades, size=n)
        want = float(sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0)))
        assert kt.exact_dot(a, b) == want
        assert abs(float(a @ b) - want) <= kt.dot_bound(a, b)
    # a dot that cancels to the last bits: b is a up to signs that nearly annihilate the sum
    a = rng.standard_normal(300)
    b = a * np.where(np.arange(300) % 2 == 0, 1.0, -1.0) * (1.0 + 2.0 ** -30 * rng.standard_normal(300))
    want = float(sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(a, b)), Fraction(0)))
    assert kt.exact_dot(a, b) == want
    assert kt.exact_dot([3.0, -2.0], [5.0, 7.0]) == 1.0 and kt.dot_bound([3.0, -2.0], [5.0, 7.0]) == kt.gamma(2) * 29.0


def test_axpy_bound_covers_the_contracted_and_the_plain_update():
    import math

    rng = np.random.default_rng(2)
    x, p = rng.standard_normal(500), rng.standard_normal(500) * 10.0 ** rng.uniform(-6, 6, size=500)
    alpha = 0.7310585786300049
    want, bound = kt.axpy_truth(x, alpha, p)
    plain = x + alpha * p
    fused = np.array([math.fsum(rtp) for rtp in zip(x.tolist(), *[v.tolist() for v in kt.rt.two_product(np.full(500, alpha), p)])])
    assert kt.within(plain, want, bound) <= 1.0 and kt.within(fused, want, bound) <= 1.0
    with pytest.raises(AssertionError):
        kt.within(x + alpha * p * (1.0 + 2.0 ** -50), want, bound)


# ------------------------------------------------------------------ the scalar phases by hand (dyadic inputs: the arithmetic below is exact)

def run(phase, rtol=0.0, hist=None, cap=0, **kw):
    return kt.scalar_phase(kt.PHASES[phase], S(**kw), rtol, hist, cap)


def test_init_and_restart_by_hand():
    s = run("init", 0.5, red=[3, 4, 9], alpha=7, beta=7, iters=5, done=-1)
    assert (s.rz, s.bb, s.rr, s.tol2, s.alpha, s.beta, s.iters, s.done) == (3, 4, 4, 1.0, 0, 0, 0, 0)
    assert run("init", 0.0, red=[3, 4, 0]).tol2 == 0.0
    s = run("init", 0.5, red=[0, 0, 0], done=0)  # b = 0: finished at once
    assert s.done == 1 and s.tol2 == 0.0 and s.bb == 0.0
    s = run("restart", red=[3, 2, 0], tol2=2, bb=16, iters=4, alpha=5)  # r.r == tol2 exactly: converged
    assert (s.rz, s.rr, s.done, s.bb, s.iters, s.alpha) == (3, 2, 1, 16, 4, 5)
    assert run("restart", red=[3, 2.0000000000000004, 0], tol2=2).done == 0
    assert run("restart", red=[3, 1, 0], tol2=2, done=-1).done == 1  # (whatever the flag was)


def test_alpha_by_hand_with_every_breakdown():
    s = run("alpha", red=[2, 0, 0], rz=3, alpha=9)
    assert s.alpha == 1.5 and s.done == 0
    for pq in (0.0, -0.0, -2.0, np.nan):
        s = run("alpha", red=[pq, 0, 0], rz=3, alpha=9)
        assert s.done == -1 and s.alpha == 9  # the old alpha stays
    assert run("alpha", red=[np.inf, 0, 0], rz=3).alpha == 0.0


def test_beta_by_hand_with_the_history_cap():
    for iters, written in ((2, True), (3, True), (4, False), (5, False)):  # iters -> it = iters + 1 against a cap of 4
        hist = np.full(6, -7.0)
        s = run("beta", hist=hist, cap=4, red=[2, 0.5, 0], rz=4, bb=8, tol2=0.25, iters=iters, beta=9)
        assert (s.beta, s.rz, s.rr, s.iters, s.done) == (0.5, 2, 0.5, iters + 1, 0)
        want = np.full(6, -7.0)
        if written:
            want[iters] = 0.0625
        np.testing.assert_array_equal(hist, want)
    s = run("beta", red=[2, 0.25, 0], rz=4, bb=8, tol2=0.25, beta=9)  # == tol2: converged, beta and rz stay; a null history
    assert (s.beta, s.rz, s.rr, s.iters, s.done) == (9, 4, 0.25, 1, 1)
    s = run("beta", red=[2, np.nan, 0], rz=4, bb=8, tol2=0.25)  # NaN is not <= tol2: the recurrence goes on (and ALPHA breaks it)
    assert s.done == 0 and s.beta == 0.5


def test_fused_init_and_fused_step_by_hand():
    s = run("fused_init", 0.5, red=[3, 4, 6], iters=3)
    assert (s.rz, s.bb, s.rr, s.tol2, s.alpha, s.beta, s.iters, s.done) == (3, 4, 4, 1.0, 0.5, 0, 0, 0)
    assert (s.ring_rz[0], s.ring_alpha[0]) == (3, 0.5)
    for zaz in (0.0, -1.0, np.nan):
        s = run("fused_init", 0.5, red=[3, 4, zaz])
        assert s.done == -1 and s.alpha == 0 and s.ring_alpha[0] == 0
    s = run("fused_init", 0.5, red=[0, 0, 0])
    assert s.done == 1  # b = 0 wins over z.Az = 0
    hist = np.full(3, -7.0)
    s = run("fused_step", hist=hist, cap=3, red=[2, 1, 8], rz=4, alpha=0.5, bb=8, tol2=0.5, iters=1)
    # beta = 2 / 4, denom = 8 - 0.5 * 2 / 0.5 = 6
    assert (s.beta, s.alpha, s.rz, s.rr, s.iters, s.done) == (0.5, 2.0 / 6.0, 2, 1, 2, 0) and hist[1] == 0.125
    for zaz in (2.0, 1.0, np.nan):  # denom = 0, < 0, NaN
        s = run("fused_step", red=[2, 1, zaz], rz=4, alpha=0.5, bb=8, tol2=0.5, beta=9)
        assert (s.done, s.beta, s.alpha, s.rz, s.iters) == (-1, 9, 0.5, 4, 1)
    s = run("fused_step", red=[2, 0.5, 8], rz=4, alpha=0.5, bb=8, tol2=0.5, beta=9)
    assert (s.done, s.beta, s.alpha, s.rz) == (1, 9, 0.5, 4)


def test_flexible_phases_by_hand_with_the_clamps():
    s = run("flex_init", 0.5, red=[4, 0, 0], pass_xx=3, pass_rhs_rr=3, rz=5, alpha=5, beta=5, iters=5)
    assert (s.bb, s.rr, s.tol2, s.rz, s.alpha, s.beta, s.iters, s.done, s.pass_xx, s.pass_rhs_rr) == (4, 4, 1, 0, 0, 0, 0, 0, 0, 0)
    assert run("flex_init", 0.5, red=[0, 0, 0]).done == 1
    s = run("flex_rz0", red=[3, 0, 0])
    assert s.rz == 3 and s.done == 0
    for rz in (0.0, -1.0, np.nan):
        assert run("flex_rz0", red=[rz, 0, 0]).done == -1
    assert run("flex_warm", red=[1, 0, 0], tol2=1).done == 1 and run("flex_warm", red=[2, 0, 0], tol2=1, done=1).done == 0
    # a refinement pass starts: rtol = 0 as cg_amg passes it, and rtol > 0
    s = run("flex_restart", 0.0, red=[4, 0, 0], bb=64, rz=5, alpha=5, beta=5, iters=9)
    assert (s.rr, s.rz, s.alpha, s.beta, s.done, s.tol2, s.pass_rhs_rr, s.iters, s.bb) == (4, 0, 0, 0, 0, 1.0e-4 * 1.0e-4 * 4, 4, 9, 64)
    assert run("flex_restart", 0.0, red=[0, 0, 0], bb=64).done == 1
    s = run("flex_restart", 0.25, red=[2, 0, 0], bb=64)  # tol2 of the solve = 4 wins over the drop of the pass
    assert (s.done, s.tol2) == (1, 4)
    # the stopping test of an iteration, flat ...
    hist = np.full(2, -7.0)
    s = run("flex_conv", hist=hist, cap=2, red=[2, 5, 0], bb=8, tol2=1, iters=0)
    assert (s.rr, s.iters, s.done, s.tol2) == (2, 1, 0, 1) and hist[0] == 0.25
    assert run("flex_conv", red=[1, 5, 0], bb=8, tol2=1).done == 1
    # ... and adaptive: drop = 0.2 rtol sqrt(xx / ee), clamped to [1e-6, 1e-2]
    for ee, d in ((1.0, 0.2 * 2.0 ** -10 * 1.0), (2.0 ** 40, 1.0e-6), (2.0 ** -40, 1.0e-2)):
        s = run("flex_conv", red=[2, ee, 0], bb=8, tol2=1, pass_xx=1, pass_rhs_rr=4, pass_rtol=2.0 ** -10)
        assert s.tol2 == d * d * 4 and s.done == (1 if 2 <= d * d * 4 else 0)
    for kw in ({"pass_xx": 0, "pass_rhs_rr": 4}, {"pass_xx": 1, "pass_rhs_rr": 0}):  # no adaptive rule without its inputs
        assert run("flex_conv", red=[2, 1, 0], bb=8, tol2=1, pass_rtol=1, **kw).tol2 == 1
    assert run("flex_conv", red=[2, 0, 0], bb=8, tol2=1, pass_xx=1, pass_rhs_rr=4, pass_rtol=1).tol2 == 1  # e = 0 so far
    s = run("flex_beta", red=[2, 8, 0], alpha=0.5, rz=4)
    assert (s.beta, s.rz, s.done) == (-1, 2, 0)
    for rz in (0.0, -1.0, np.nan):
        s = run("flex_beta", red=[rz, 8, 0], alpha=0.5, rz=4, beta=9)
        assert (s.done, s.beta, s.rz) == (-1, 9, 4)


def test_the_gate_rule():
    for name, phase in kt.PHASES.items():
        ungated = name in ("init", "restart", "fused_init", "flex_init", "flex_restart", "flex_warm")
        assert kt.gated(phase, 0) is False
        assert kt.gated(phase, 1) is (not ungated) and kt.gated(phase, -1) is (not ungated)


def test_the_folded_step_is_fused_step_through_the_ring():
    for par in (0, 1):
        for red in ([2, 1, 8], [2, 0.5, 8], [2, 1, 2], [2, 1, np.nan]):
            base = S(red=red, rz=4, alpha=0.5, bb=8, tol2=0.5, iters=3, beta=9)
            base.ring_rz[par], base.ring_alpha[par] = 4, 0.5
            base.ring_rz[par ^ 1], base.ring_alpha[par ^ 1] = 1024, 1024  # what a wrong parity would read
            h1, h2 = np.full(5, -7.0), np.full(5, -7.0)
            want = kt.scalar_phase(kt.FUSED_STEP, base.copy(), 0.0, h1, 5)
            got = base.copy()
            alpha, beta, done = kt.folded_step(got, par, h2, 5)
            kt.assert_scalars_equal(got, want, fields=kt.SCALAR_FIELDS)
            np.testing.assert_array_equal(h1, h2)
            assert done == want.done
            if done == 0:
                assert (alpha, beta) == (want.alpha, want.beta)
                assert (got.ring_rz[par ^ 1], got.ring_alpha[par ^ 1]) == (want.rz, want.alpha)
                assert (got.ring_rz[par], got.ring_alpha[par]) == (4, 0.5)
            else:
                assert (got.ring_rz[par ^ 1], got.ring_alpha[par ^ 1]) == (1024, 1024)
    done = S(done=1, red=[2, 1, 8], iters=3)
    assert kt.folded_step(done, 0) == (None, None, 1) and done.iters == 3


# ------------------------------------------------------------------ the recurrences

@pytest.fixture(scope="module")
def system():
    """K (SPD on the free dofs, unit rows on the fixed ones), F and the block-Jacobi inverse of a 42-node curved patch"""
    m = sections.curved_patch(6, 5)
    r, c, v, F = oracle.assemble(m.xyz, m.tri, np.zeros((0, 4), np.int32), oracle.material(0.3, 2e5, 0.05), m.dirichlet_mask(), m.loads)
    A = oracle.to_scipy(r, c, v)
    D = np.array([v[r[a] + list(c[r[a]:r[a + 1]]).index(a)] for a in range(len(r) - 1)])
    Dinv = np.linalg.inv(D)
    Minv = lambda x: np.einsum("nij,nj->ni", Dinv, x.reshape(-1, 6)).reshape(-1)  # noqa: E731
    return (r, c, v), A, F, Minv


def test_the_restated_classic_recurrence_gives_the_oracles_history(system):
    K, A, F, Minv = system
    x, hist, s = kt.classic(A, Minv, F, 1e-10, 2000)
    xo, info = oracle.pcg(*K, F, rtol=1e-10, max_it=2000, history=True)
    assert s.done == 1 and s.iters == len(hist) and abs(s.iters - info["iterations"]) <= 2
    k = min(40, len(hist), len(info["history"]))
    np.testing.assert_allclose(np.sqrt(hist[:k]), info["history"][:k], rtol=1e-6)
    assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)
    assert (hist[:-1] > s.tol2 / s.bb).all() and hist[-1] * s.bb <= s.tol2 * (1 + 1e-15)
    # the iteration limit ends it with done = 0 and as many history words
    x9, h9, s9 = kt.classic(A, Minv, F, 0.0, 9)
    assert (s9.done, s9.iters, len(h9)) == (0, 9, 9)
    np.testing.assert_array_equal(h9, kt.classic(A, Minv, F, 1e-10, 2000)[1][:9])


def test_the_single_reduction_recurrence_folded_is_the_unfolded_one_bit_for_bit(system):
    K, A, F, Minv = system
    xc, hc, _ = kt.classic(A, Minv, F, 1e-10, 2000)
    for rtol, max_it in ((1e-10, 2000), (0.0, 1), (0.0, 2), (0.0, 9), (0.0, 17)):
        xf, hf, sf = kt.single_reduction(A, Minv, F, rtol, max_it, fold=True)
        xu, hu, su = kt.single_reduction(A, Minv, F, rtol, max_it, fold=False)
        np.testing.assert_array_equal(xf, xu)
        np.testing.assert_array_equal(hf, hu)
        kt.assert_scalars_equal(sf, su, fields=kt.SCALAR_FIELDS)
        assert sf.iters == len(hf) == (max_it if rtol == 0.0 else sf.iters)
        k = min(30, len(hf))
        np.testing.assert_allclose(hf[:k], hc[:k], rtol=1e-5)  # the classic iterates, in exact arithmetic
    assert sf.done == 0 and kt.single_reduction(A, Minv, F, 1e-10, 2000)[2].done == 1


def test_the_restated_flexible_recurrence_gives_the_oracles_history(system):
    from oracle import amg_oracle

    K, A, F, Minv = system
    x, hist, s = kt.flexible(A, Minv, F, 1e-10, 2000)
    xo, ho = amg_oracle.flexible_pcg(A, F, Minv, rtol=1e-10, max_it=2000)
    assert s.done == 1 and abs(len(hist) - len(ho)) <= 2
    k = min(40, len(hist), len(ho))
    np.testing.assert_allclose(np.sqrt(hist[:k]), ho[:k], rtol=1e-6)
    assert np.linalg.norm(x - xo) <= 1e-8 * np.linalg.norm(xo)
    # a positive definite preconditioner that is not: the breakdown branch of FLEX_RZ0
    assert kt.flexible(A, lambda r: -r, F, 1e-10, 10)[2].done == -1
    assert kt.flexible(A, Minv, np.zeros_like(F), 1e-10, 10)[2].done == 1


# ------------------------------------------------------------------ the reduction model and the planted defects

@pytest.mark.parametrize("n", kt.REDUCE_LENGTHS)
def test_reduce_model_adds_integers_exactly_and_anything_within_the_bound(n):
    rng = np.random.default_rng(n)
    assert kt.reduce_groups(n) == (64 if n >= 4096 else 1)
    p = kt.integer_partials(n)
    kt.assert_reduction_exact(kt.reduce_model(p), p)
    for i in kt.chunk_edges(n):
        assert kt.reduce_model(kt.one_hot(n, i)) == 1.0
    for p in (kt.random_partials(rng, n), kt.cancelling(rng, n)):
        kt.assert_reduction_within(kt.reduce_model(p), p)
    c = kt.cancelling(rng, n)
    if n >= 255:
        assert abs(kt.exact_sum(c)) <= 1e-11 * float(np.abs(c).sum())


@pytest.mark.parametrize("n", [4096, 4097, 8232, 65536])
def test_a_reduction_that_drops_its_last_chunk_is_caught(n):
    rng = np.random.default_rng(n)
    p = kt.integer_partials(n)
    with pytest.raises(AssertionError, match="difference"):
        kt.assert_reduction_exact(kt.reduce_model(p, defect="drop_last_chunk"), p)
    assert kt.reduce_model(kt.one_hot(n, n - 1), defect="drop_last_chunk") == 0.0  # the one-hot case of the GPU test reads 1.0
    p = kt.random_partials(rng, n)
    with pytest.raises(AssertionError):
        kt.assert_reduction_within(kt.reduce_model(p, defect="drop_last_chunk"), p)


def test_a_symmetric_fused_dot_that_counts_the_in_slice_products_twice_is_caught(system):
    K, A, F, Minv = system
    rng = np.random.default_rng(3)
    for x in (rng.standard_normal(len(F)), kt.small_integers(rng, len(F))):
        truth, extra = kt.fused_dot_truth(K, x)
        assert abs(truth - float(x @ (A @ x))) <= 1e-9 * abs(truth)
        kt.assert_dot([kt.sym_fused_dot_model(K, x)], x, A @ x, truth=truth, bound=extra)
        with pytest.raises(AssertionError):
            kt.assert_dot([kt.sym_fused_dot_model(K, x, defect="in_slice_twice")], x, A @ x, truth=truth, bound=extra)


def test_a_dot_that_includes_a_ghost_row_is_caught():
    rng = np.random.default_rng(4)
    n_owned, n_ghost = 40, 5
    for make in (lambda: rng.standard_normal(6 * (n_owned + n_ghost)), lambda: kt.small_integers(rng, 6 * (n_owned + n_ghost)) + 4.0):
        a, b = make(), make()
        own = slice(0, 6 * n_owned)
        kt.assert_dot([kt.owned_dot_model(a, b, n_owned)], a[own], b[own])
        with pytest.raises(AssertionError):
            kt.assert_dot([kt.owned_dot_model(a, b, n_owned, defect="ghost_row")], a[own], b[own])


def test_a_folded_step_that_reads_the_wrong_ring_parity_is_caught(system):
    K, A, F, Minv = system
    # the state two iterations in, as the GPU test sets it: the halves of the ring differ as they do in every solve
    _, _, s = kt.single_reduction(A, Minv, F, 0.0, 2, fold=True)
    assert s.ring_rz[0] != s.ring_rz[1] and s.ring_alpha[0] != s.ring_alpha[1]
    for par in (0, 1):
        base = s.copy()
        base.ring_rz[par], base.ring_alpha[par] = base.rz, base.alpha  # the half this step reads holds what FUSED_STEP keeps in rz / alpha
        base.red = np.array([0.5 * float(base.rz), 0.25 * float(base.rr), 3.0 * float(base.rz) / float(base.alpha)])
        want = kt.scalar_phase(kt.FUSED_STEP, base.copy(), 0.0)
        got = base.copy()
        kt.folded_step(got, par)
        kt.assert_scalars_equal(got, want, fields=kt.SCALAR_FIELDS)
        bad = base.copy()
        kt.folded_step(bad, par, defect="wrong_parity")
        with pytest.raises(AssertionError):
            kt.assert_scalars_equal(bad, want, fields=kt.SCALAR_FIELDS)
    # ... and a chained solve leaves the unfolded one's at the first folded step: it reads the half of the ring nobody has written
    # yet, zeros, and breaks down
    hu = kt.single_reduction(A, Minv, F, 0.0, 9, fold=False)[1]
    _, hb, sb = kt.single_reduction(A, Minv, F, 0.0, 9, fold=True, defect="wrong_parity")
    assert hu[0] == hb[0] and (sb.done, len(hb)) == (-1, 1) and len(hu) == 9
