"""The inputs and references of tests/test_gpu_dense_inverse.py, proven without a GPU: the long-double truth against exact
rational answers, the plain-double restatement of the sweep method and the host's Cholesky inverse
(femshell_amg_host_dense_inverse) against that truth, the planted dead directions and the verdicts either side of the two
pivot rules, and the tile map of the trailing update (every lower tile exactly once).  CPU only."""
import importlib
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import dense_truth as dt
from tests.helpers.product import ensure_built

LD = dt.LD
PLANTED = [(43, (70,)), (43, (5, 6)), (43, (130, 200)), (43, (257,))]  # n = 258


def _binding():
    ensure_built()
    return importlib.import_module("fem-shell_amd.binding")


def _host(A):
    return _binding().amg_host_dense_inverse(*dt.to_block_csr(A))


def _rational_inverse(A):
    n = len(A)
    M = [[Fraction(int(A[i][j])) for j in range(n)] + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        p = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[p] = M[p], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                M[r] = [a - M[r][c] * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


def test_truth_equals_the_rational_inverse_of_an_integer_matrix():
    rng = np.random.default_rng(12)
    G = rng.integers(-3, 4, size=(12, 20))
    A = (G @ G.T).astype(np.float64)
    exact = _rational_inverse(A)
    X = dt.truth_inverse(A)
    # entry by entry against the rational number rounded once to long double; the truth may be off by cond x 2^-64 x a few
    E = np.array([[LD(v.numerator) / LD(v.denominator) for v in row] for row in exact], dtype=LD)
    cond = np.linalg.cond(A)
    assert cond < 1e4
    assert dt.err(X, E) <= 64 * cond * 2.0 ** -64, (dt.err(X, E), cond)
    # and the Newton step leaves an exact answer where it is: forced by an unreachable `need`
    info = {}
    X2 = dt.truth_inverse(A, need=0.0, info=info)
    assert info["newton"] and dt.err(X2, E) <= 64 * cond * 2.0 ** -64


def _cases():
    out = [("a", 21, dt.random_spd(21)), ("a", 43, dt.random_spd(43)), ("b", 22, dt.graded(22)), ("b", 65, dt.graded(65))]
    for kind in ("panel", "roof"):
        out.append(("c-" + kind, None, dt.from_block_csr(*dt.galerkin(kind))))
    return out


@pytest.fixture(scope="module")
def cases():
    ensure_built()
    return _cases()


def test_truth_defect_restatement_and_host_entry_on_the_positive_definite_families(cases):
    for fam, nodes, A in cases:
        n = len(A)
        assert np.array_equal(A, A.T) or fam.startswith("c")
        As = 0.5 * (A + A.T)  # (the host symmetrises, the device reads the lower triangle: the Galerkin product differs in the 16th digit)
        R, dropped, failed = dt.restated_inverse(As)
        assert failed is None and dropped == [], (fam, nodes, dropped, failed)
        lap = np.linalg.inv(As)
        info = {}
        rough = float(np.abs(R - lap).max() / np.abs(lap).max())
        X = dt.truth_inverse(As, need=rough, info=info)
        cond = np.linalg.cond(As)
        e_r, e_l, e_h = dt.err(R, X), dt.err(lap, X), dt.err(_host(A), X)
        print("%-8s n=%4d cond %.1e truth defect %.1e own %.1e newton %d | restated %.2e lapack %.2e host %.2e"
              % (fam, n, cond, info["defect"], info["own_error"], info["newton"], e_r, e_l, e_h))
        # the truth: its long-double defect is cond x n x 2^-64 at the most, and it stands 100 x below what it judges
        assert info["defect"] <= n * cond * 2.0 ** -64, (fam, info)
        assert info["newton"] or info["own_error"] * 100.0 <= rough
        # the double paths: backward-stable inverses of a matrix of this condition number
        for name, e in (("restated", e_r), ("lapack", e_l), ("host", e_h)):
            assert e <= 8 * cond * dt.U, (fam, nodes, name, e, cond)
        # the restatement sits at LAPACK's level and the host's Cholesky at the restatement's: each within the project's margin
        assert e_r <= dt.bound(e_l, n) and e_h <= dt.bound(e_r, n), (fam, e_r, e_l, e_h)
        assert np.array_equal(R, R.T)


def test_galerkin_family_is_a_real_coarse_operator():
    for kind in ("panel", "roof"):
        rp, ci, vals = dt.galerkin(kind)
        n = 6 * (len(rp) - 1)
        A = dt.from_block_csr(rp, ci, vals)
        assert n >= 6 * 30 and rp[-1] < (len(rp) - 1) ** 2  # sparse, and beyond one pivot block
        assert np.abs(A - A.T).max() <= 1e-12 * np.abs(A).max() and np.linalg.eigvalsh(0.5 * (A + A.T)).min() > 0.0


@pytest.mark.parametrize("nodes,dead", PLANTED)
def test_planted_dead_directions_are_dropped_and_the_rest_is_the_truth(nodes, dead):
    A = dt.planted(nodes, dead)
    n = len(A)
    R, dropped, failed = dt.restated_inverse(A)
    assert failed is None and dropped == sorted(dead)
    X = dt.embedded_truth(A, dead)
    H = _host(A)
    e_r, e_h = dt.err(R, X), dt.err(H, X)
    keep = np.setdiff1d(np.arange(n), dead)
    cond = np.linalg.cond(A[np.ix_(keep, keep)])
    print("planted %s n=%d cond of the kept part %.1e restated %.2e host %.2e" % (dead, n, cond, e_r, e_h))
    assert cond < 1e3 and e_r <= 8 * cond * dt.U and e_h <= dt.bound(e_r, n)
    for Y in (R, H):
        assert not Y[list(dead), :].any() and not Y[:, list(dead)].any()
    assert sorted(np.nonzero(np.diag(H) == 0.0)[0]) == sorted(dead)  # the host drops exactly the planted set


@pytest.mark.parametrize("rel,kept", [(1e-9, True), (1e-13, False)])
def test_verdict_two_decades_either_side_of_the_drop_threshold(rel, kept):
    p = 70
    A = dt.near_threshold(43, p, rel)
    R, dropped, failed = dt.restated_inverse(A)
    assert failed is None and dropped == ([] if kept else [p])
    H = _host(A)
    assert (H[p, p] != 0.0) == kept and (np.diag(H) == 0.0).sum() == (0 if kept else 1)


@pytest.mark.parametrize("p", [70, 200])
def test_clearly_negative_pivot_and_zero_diagonal_are_breakdowns(p):
    b = _binding()
    for A, where in ((dt.clearly_negative(43, p), p), (dt.zero_diagonal(43, p), p)):
        R, dropped, failed = dt.restated_inverse(A)
        assert R is None and failed == where
        with pytest.raises(b.FemShellError) as e:
            b.amg_host_dense_inverse(*dt.to_block_csr(A))
        assert e.value.code == dt.BREAKDOWN


def test_block_restatement_shows_what_explicit_pivot_block_inverses_cost():
    """The device forms the inverses of its pivot blocks explicitly (groups of four pivots, 64-halves, the 128-wide block); restated
    with that structure in plain double the method stays at the scalar sweep's level on well-conditioned pivot blocks and loses
    cond(pivot block) u on graded ones -- on the CPU, without the device: the loss belongs to the arithmetic."""
    for fam, which in (("a", 22), ("c", "roof"), ("d", (43, (130, 200))), ("d", (40, (5, 6)))):
        c = dt.case(fam, which)
        assert c["e_block"] <= dt.bound(c["e_restated"], c["n"]), (fam, which, c["e_block"], c["e_restated"])
    for nodes in (11, 22, 32):
        c = dt.case("b", nodes)
        print("b-%d scalar %.2e block %.2e cond(pivot block) u %.2e" % (nodes, c["e_restated"], c["e_block"], c["kappa_pivot"] * dt.U))
        assert c["e_block"] >= 100.0 * c["e_restated"], (nodes, c["e_block"], c["e_restated"])
        assert c["e_block"] <= 8.0 * c["kappa_pivot"] * dt.U, (nodes, c["e_block"], c["kappa_pivot"])
        assert c["bound"] == dt.bound(max(c["e_block"], c["kappa_pivot"] * dt.U), c["n"])
    # the verdicts of the block restatement are the scalar one's
    for rel, dropped in ((1e-9, 0), (1e-13, 1)):
        assert dt.restated_block_inverse(dt.near_threshold(43, 200, rel))[1:] == (dropped, 0)
    assert dt.restated_block_inverse(dt.clearly_negative(43, 200))[2] == 1


@pytest.mark.parametrize("nt", [2, 4, 6, 8, 10, 12, 18, 26, 116])
def test_tile_map_lists_every_lower_tile_exactly_once(nt):
    lists = _binding().amg_host_dense_tile_map(nt)
    np.testing.assert_array_equal(lists, dt.tile_map_model(nt))
    counts = dt.tiles_of_map(lists, nt)
    np.testing.assert_array_equal(counts, np.tril(np.ones((nt, nt), dtype=np.int64)))
    # a super-block belongs to one XCD, and the lists are balanced to one super-block's weight
    flat = lists[lists >= 0]
    assert len(np.unique(flat)) == len(flat) == ((nt + 7) // 8) * ((nt + 7) // 8 + 1) // 2
    load = [sum(int(dt.tiles_of_map(np.array([[sb]] + [[-1]] * 7, dtype=np.int32), nt).sum()) for sb in row if sb >= 0) for row in lists]
    assert max(load) - min(load) <= 64


def test_new_entry_points_are_bound():
    b = _binding()
    for name in ("femshell_amg_device_dense_inverse", "femshell_amg_dense_apply", "femshell_amg_symbolic_info"):
        assert name in b.SYMBOLS and getattr(b.load_library(), name).argtypes is not None
