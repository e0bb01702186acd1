"""The restatement of the load cases' lockstep recurrence (tests/helpers/load_cases.py), pinned on the CPU: against a dense solve
of an oracle-assembled K, by the properties the device is held to -- a column does not depend on its company -- and by planted
defects that those checks must catch.  No GPU, no library."""
import numpy as np
import pytest

from tests.helpers import load_cases as lc, oracle, prescribed as pr

NU, E, T = 0.3, 2.1e5, 0.37
LD = lc.LD


@pytest.fixture(scope="module")
def strip():
    """strip33 under the mask of the GPU tests: (K dense in float64, D^-1, B (7, n) masked, the dense solutions in long double)"""
    xyz, tri = pr.strip33()
    mask = lc.mask_of(len(xyz))
    rowptr, colidx, vals, _ = oracle.assemble(xyz, tri, np.zeros((0, 4), np.int32), oracle.material(NU, E, T), mask, None)
    K = lc.dense_from_bsr(rowptr, colidx, vals)
    assert np.array_equal(K, K.T) or np.abs(K - K.T).max() <= 1e-12 * np.abs(K).max()
    B = np.where(lc.free_dofs(mask), lc.case_loads(len(xyz), mask, 7).reshape(7, -1), 0.0)
    return K, lc.block_jacobi(K), B, lc.dense_solve(K, B)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a - b, dtype=LD)) / np.linalg.norm(np.asarray(b, dtype=LD)))


def test_scalar_step_by_hand():
    s = lc.Column()
    assert lc.scalar_step(lc.INIT, s, (LD(3), LD(4)), 0.5)
    assert (s.rz, s.bb, s.rr, s.tol2, s.alpha, s.beta, s.iters, s.done) == (3, 4, 4, 1, 0, 0, 0, 0)
    assert lc.scalar_step(lc.ALPHA, s, (LD(6),), 0.5) and s.alpha == LD(0.5) and s.pq == 6 and s.done == 0
    assert lc.scalar_step(lc.BETA, s, (LD(1.5), LD(2)), 0.5) and (s.beta, s.rz, s.rr, s.iters, s.done) == (0.5, 1.5, 2, 1, 0)
    assert lc.scalar_step(lc.BETA, s, (LD(9), LD(1)), 0.5) and (s.beta, s.rz, s.rr, s.iters, s.done) == (0.5, 1.5, 1, 2, 1)
    # frozen: no step but INIT touches a finished column
    before = dict(s.__dict__)
    assert not lc.scalar_step(lc.ALPHA, s, (LD(1),), 0.5) and not lc.scalar_step(lc.BETA, s, (LD(1), LD(1)), 0.5)
    assert s.__dict__ == before
    # rtol <= 0: the threshold is zero, only an exact zero residual stops; b = 0 is done at once
    z = lc.Column()
    lc.scalar_step(lc.INIT, z, (LD(3), LD(4)), 0.0)
    assert z.tol2 == 0 and z.done == 0
    lc.scalar_step(lc.INIT, z, (LD(0), LD(0)), 1e-8)
    assert z.done == 1 and z.iters == 0
    for pq in (0.0, -1.0, np.nan):
        b = lc.Column()
        lc.scalar_step(lc.INIT, b, (LD(3), LD(4)), 0.5)
        lc.scalar_step(lc.ALPHA, b, (LD(pq),), 0.5)
        assert b.done == -1 and b.alpha == 0


def test_restatement_against_the_dense_solve(strip):
    """seven cases in passes of four to rtol 1e-13: every column agrees with np.linalg.solve (refined in long double) far below the
    tolerance times the condition of the strip; the zero case returns zeros in no iteration; at least two columns of the first
    pass stop at different iterations"""
    K, Minv, B, U = strip
    X, cols, passes = lc.lockstep(K, Minv, B, 1e-13, 2000)
    assert passes == 2
    for j, s in enumerate(cols):
        if j == 2:
            assert s.done == 1 and s.iters == 0 and not X[j].any()
            continue
        assert s.done == 1 and 0 < s.iters < 2000
        assert rel(X[j], U[j]) <= 1e-9, (j, rel(X[j], U[j]))
    assert len({cols[j].iters for j in (0, 1, 3)}) > 1


def test_a_column_does_not_depend_on_its_company(strip):
    """bit for bit in float64: alone, in every position of a pass, in the tail pass, with rtol = 0 and few iterations too"""
    K, Minv64, B, _ = strip[0], lc.block_jacobi(strip[0], np.float64), strip[2], None
    for rtol, max_it in ((1e-10, 2000), (0.0, 1), (0.0, 2), (0.0, 5)):
        alone = [lc.lockstep(K, Minv64, B[j:j + 1], rtol, max_it, dtype=np.float64) for j in range(7)]
        for order in ([0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0], [1, 0], [3, 1, 4], [2, 2, 0, 1, 5]):
            X, cols, _ = lc.lockstep(K, Minv64, B[order], rtol, max_it, dtype=np.float64)
            for k, j in enumerate(order):
                assert np.array_equal(X[k], alone[j][0][0]) and cols[k].iters == alone[j][1][0].iters, (rtol, max_it, order, k)
                if rtol == 0.0 and j != 2:
                    assert cols[k].iters == max_it and cols[k].done == 0


def test_scaling_by_a_power_of_two_is_exact(strip):
    K, B = strip[0], strip[2]
    Minv64 = lc.block_jacobi(K, np.float64)
    X, cols, _ = lc.lockstep(K, Minv64, np.stack([B[0], 1024.0 * B[0]]), 1e-10, 2000, dtype=np.float64)
    assert np.array_equal(1024.0 * X[0], X[1]) and cols[0].iters == cols[1].iters


@pytest.mark.parametrize("defect", lc.DEFECTS)
def test_planted_defects_are_caught(strip, defect):
    """each defect fails the dense solve or the independence of a column, the two checks the device is held to"""
    K, Minv, B, U = strip
    Bd = B[:5]
    with np.errstate(all="ignore"):  # (a column on a foreign alpha may diverge)
        X, cols, _ = lc.lockstep(K, Minv, Bd, 1e-13, 2000, defect=defect)
    good, _, _ = lc.lockstep(K, Minv, Bd, 1e-13, 2000)
    assert max(rel(good[j], U[j]) for j in (0, 1, 3, 4)) <= 1e-9
    wrong_solution = max(rel(X[j], U[j]) for j in (0, 1, 3, 4)) > 1e-6
    alone = [lc.lockstep(K, Minv, Bd[j:j + 1], 1e-13, 2000, defect=defect)[0][0] for j in range(5)]
    depends_on_company = any(not np.array_equal(X[j], alone[j]) for j in range(5))
    print("defect %-24s wrong solution %s, depends on company %s" % (defect, wrong_solution, depends_on_company))
    assert wrong_solution or depends_on_company
    if defect == "tail_pass_fifth_column":
        assert not X[4].any()  # never read
    if defect == "alpha_of_column_0":
        assert np.array_equal(X[0], good[0]) and not np.array_equal(X[1], good[1])
    if defect == "update_after_done":
        # the steps a converged column goes on taking are of the size of its last one: far below what the dense solve sees, which is
        # why the device is compared bit for bit with the column solved alone
        assert depends_on_company and not wrong_solution


def test_breakdown_freezes_that_column_only():
    """p.Ap <= 0 in one column sets its done to -1 and freezes it; the other column finishes.  Shown on the restatement with an
    indefinite system of two 2 x 2 blocks: the stiffness of a supported shell is positive definite, so no context reaches this
    branch and the device is not tested for it."""
    A = np.zeros((4, 4))
    A[:2, :2] = [[4.0, 1.0], [1.0, 3.0]]
    A[2:, 2:] = [[1.0, 2.0], [2.0, 1.0]]  # eigenvalues 3 and -1

    def Minv(r):
        return np.asarray(r, dtype=LD)

    B = np.array([[1.0, 2.0, 0.0, 0.0], [0.0, 0.0, 1.0, -1.0], [1.0, -1.0, 0.0, 0.0]])
    X, cols, _ = lc.lockstep(A, Minv, B, 1e-14, 50)
    assert [s.done for s in cols] == [1, -1, 1]
    assert cols[1].iters == 0 and cols[1].pq < 0 and not X[1].any()  # (1, -1) is the eigenvector of -1: the first p.Ap is negative
    for j in (0, 2):
        assert rel(X[j][:2], np.linalg.solve(A[:2, :2], B[j][:2]).astype(LD)) <= 1e-14 and cols[j].iters <= 2
    # alone, the good columns give the same bits
    for j in (0, 2):
        assert np.array_equal(lc.lockstep(A, Minv, B[j:j + 1], 1e-14, 50)[0][0], X[j])
