"""The double-double residual r = F - K x (k_residual_dd, k_residual_dd_sym in csrc/spmv_kernels.hip) against an exact truth, row
by row: the truth, the error budget, and a restatement of the kernels' arithmetic that takes planted defects.

K is the exported block matrix, (rowptr, colidx, vals[nb, 6, 6]) of export_bsr() (longer tuples are cut), F and x have six values
per node.  numpy and the standard library only.

exact   the correctly rounded value of F_i - sum_j K_ij x_j per scalar row: every product as an error-free pair p + e = a x
        (Dekker's product on Veltkamp's split), the row summed by math.fsum over F_i, the -p and the -e, which is exact and
        rounds once.  fraction() is the same number by rational arithmetic, for the pin.
bound   u |r*_i| + gamma_m^2 S_i with u = 2^-53, S_i = |F_i| + (|K||x|)_i, m = 6 (blocks in row i) + 2,
        gamma_m = m u / (1 - m u): the bound of Dot2 (Ogita, Rump, Oishi, Accurate sum and dot product, SIAM J. Sci. Comput. 26
        (2005), Prop. 5.5).  The kernels are that algorithm -- TwoProduct, TwoSum of the running sum and the product, the two
        error terms added to a second accumulator in plain FP64 -- over the 6 (blocks) products of a row; F_i is one more exact
        term and the closing b - (hi + lo) takes the part of Dot2's last addition: m - 1 terms and one.  A padded slot is a
        product of zeros: exact zeros in both accumulators, no term.  The bound holds for every order of the terms.  Derived,
        not measured; S is summed in long double and rounded once, a relative 1e-19 of a bound the intact arithmetic uses a
        few percent of.
model   dd_fma_acc and the closing step in numpy, all rows at once, a term per step; defect= plants one of DEFECTS.

states() builds the inputs the tests run: "cancel" (F = fl(K x): the exact residual is the rounding noise of that product),
"zero" (F = 0, the way tests/helpers/manufactured.py uses the kernel), "free" (K x of the size of F, no cancellation: the input
the older tests use)."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SPLITTER = 134217729.0  # 2^27 + 1
# operands of a product inside [2^-450, 2^450] (or zero): the split cannot overflow, and the smallest bit any partial product can
# hold, 2^-104 |a| |x| >= 2^-1004, is a normal number -- no underflow anywhere in the error-free product
OPERAND_MIN, OPERAND_MAX = 2.0 ** -450, 2.0 ** 450

DEFECTS = ("transposed_e", "contracted", "no_lo", "fp64")


def _bsr(K):
    rowptr, colidx, vals = (np.asarray(a) for a in K[:3])
    return rowptr.astype(np.int64), colidx.astype(np.int64), np.asarray(vals, dtype=np.float64).reshape(-1, 6, 6)


def blocks_per_row(K):
    """blocks in the node row of every scalar row"""
    return np.repeat(np.diff(_bsr(K)[0]), 6)


def terms(K, x, order="stored"):
    """(A, X, lower): the factors of every scalar row's products, a term per leading index -- A[t, i] x X[t, i] is the t-th term
    of row i, exact zeros behind the row's last block; lower[t, i]: the term's column node is below the row's node (with
    symmetric storage that half is not stored: the kernel takes it from the transposed block of the in-list).
    order: "stored" -- ascending column node, as k_residual_dd walks a row; "sym" -- the diagonal block, the blocks right of it,
    then the blocks left of it, as k_residual_dd_sym does (own row first, in-list after)."""
    rowptr, colidx, vals = _bsr(K)
    n = len(rowptr) - 1
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    assert len(x) == 6 * n and (n == 0 or colidx.max() < n)
    d = np.diff(rowptr)
    W = int(d.max())
    k = np.arange(W)[None, :]
    src = np.broadcast_to(k, (n, W))
    if order == "sym":
        node = np.repeat(np.arange(n), d)
        n_lower = np.bincount(node, weights=(colidx < node), minlength=n).astype(np.int64)[:, None]
        n_upper = d[:, None] - n_lower - 1
        assert np.all(colidx[rowptr[:-1] + n_lower[:, 0]] == np.arange(n))  # every row has its diagonal block, columns ascend
        src = np.where(k == 0, n_lower, np.where(k <= n_upper, n_lower + k, k - n_upper - 1))
    else:
        assert order == "stored"
    live = k < d[:, None]
    q = np.where(live, rowptr[:-1, None] + src, len(colidx))  # the zero block appended below
    vals = np.concatenate([vals, np.zeros((1, 6, 6))])
    cols = np.concatenate([colidx, [n]])
    x6 = np.concatenate([x.reshape(n, 6), np.zeros((1, 6))])
    A = vals[q].transpose(0, 2, 1, 3).reshape(6 * n, 6 * W)  # [node, i, slot, j]
    X = np.broadcast_to(x6[cols[q]][:, None, :, :], (n, 6, W, 6)).reshape(6 * n, 6 * W)
    lower = np.broadcast_to((live & (cols[q] < np.arange(n)[:, None]))[:, None, :, None], (n, 6, W, 6)).reshape(6 * n, 6 * W)
    return np.ascontiguousarray(A.T), np.ascontiguousarray(X.T), np.ascontiguousarray(lower.T)


def _split(a):
    c = SPLITTER * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(p, e) with p = fl(a b) and a b = p + e exactly (Dekker); the operands are asserted into the range where that holds"""
    for v in (a, b):
        nz = np.abs(v[v != 0.0])
        assert np.all(np.isfinite(v)) and (nz.size == 0 or (nz.min() >= OPERAND_MIN and nz.max() <= OPERAND_MAX))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, al * bl - (((p - ah * bh) - al * bh) - ah * bl)


def exact(K, F, x):
    """the correctly rounded F_i - sum_j K_ij x_j of every scalar row"""
    A, X, _ = terms(K, x)
    P, E = two_product(A, X)
    F = np.asarray(F, dtype=np.float64).reshape(-1)
    assert np.all(np.isfinite(F))
    rows = np.concatenate([F[None, :], -P, -E]).T
    return np.array([math.fsum(r) for r in rows.tolist()])


def fraction(K, F, x, rows):
    """the same by rational arithmetic on the given scalar rows (int / int division rounds correctly)"""
    rowptr, colidx, vals = _bsr(K)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    out = []
    for i in rows:
        a, ii = divmod(int(i), 6)
        s = Fraction(float(F[i]))
        for q in range(rowptr[a], rowptr[a + 1]):
            for j in range(6):
                s -= Fraction(float(vals[q, ii, j])) * Fraction(float(x[6 * colidx[q] + j]))
        out.append(float(s))
    return np.array(out)


def scale(K, F, x):
    """S_i = |F_i| + (|K||x|)_i"""
    A, X, _ = terms(K, x)
    ld = np.longdouble
    absF = np.abs(np.asarray(F, dtype=np.float64).reshape(-1)).astype(ld)
    return (absF + np.abs(A.astype(ld) * X.astype(ld)).sum(axis=0)).astype(np.float64)


def gamma(m):
    m = np.asarray(m, dtype=np.float64)
    assert np.all(m * U < 1.0)
    return m * U / (1.0 - m * U)


def bound(K, F, x, truth=None):
    """the budget of every scalar row (truth: exact(K, F, x) where the caller has it already)"""
    truth = exact(K, F, x) if truth is None else truth
    g = gamma(6.0 * blocks_per_row(K) + 2.0)
    return U * np.abs(truth) + g * g * scale(K, F, x)


def ratios(r, truth, budget):
    """|r - truth| / budget per row; a row whose budget is zero (no term, F_i = 0) must be exact"""
    err = np.abs(np.asarray(r, dtype=np.float64).reshape(-1) - truth)
    out = np.zeros_like(err)
    pos = budget > 0.0
    out[pos] = err[pos] / budget[pos]
    out[~pos & (err > 0.0)] = np.inf
    return out


_fused = np.frompyfunc(lambda h, p, e: math.fsum((h, p, e)), 3, 1)  # fl(h + a x) with a x = p + e: one rounding


def model(K, F, x, defect=None, order="stored"):
    """The kernels' arithmetic (dd_fma_acc per term, then r = b - (hi + lo) with b - hi taken exactly), all rows at once.
    defect: None, or
      "transposed_e"  the product error e is dropped where the column node is below the row node (the in-list half)
      "contracted"    the running sum is fl(hi + a x), one rounding -- what the backend made of hi + fl(a x) before the product
                      went through inline assembly -- while err is computed as written, from p = fl(a x)
      "no_lo"         the closing step leaves lo out
      "fp64"          plain FP64: fl(b - hi), hi the sum of the rounded products in order"""
    assert defect is None or defect in DEFECTS
    A, X, lower = terms(K, x, order)
    P, E = two_product(A, X)
    b = np.asarray(F, dtype=np.float64).reshape(-1)
    hi, lo = np.zeros_like(b), np.zeros_like(b)
    for t in range(len(A)):
        p, e = P[t], E[t]
        if defect == "fp64":
            hi = hi + p
            continue
        s = _fused(hi, p, e).astype(np.float64) if defect == "contracted" else hi + p
        bb = s - hi
        err = (hi - (s - bb)) + (p - bb)
        if defect == "transposed_e":
            e = np.where(lower[t], 0.0, e)
        hi = s
        lo = lo + (err + e)
    s = b - hi
    if defect == "fp64":
        return s
    bb = s - b
    err = (b - (s - bb)) + (-hi - bb)
    return s + err if defect == "no_lo" else s + (err - lo)


def norm_tolerance(n_dofs):
    """true_rel_residual = sqrt(sum r_i^2 / sum F_i^2) in FP64 against the same from exact numbers rounded once: each sum of N
    non-negative terms (squares rounded, then N - 1 additions in any grouping) is within (N + 1) u relative, the quotient adds u, the
    root halves and adds u, and the comparison value carries the same: 4 (N + 4) u covers both sides"""
    return 4.0 * (n_dofs + 4) * U


# ------------------------------------------------------------------ inputs

STATES = ("cancel", "zero", "free")


def csr(K):
    """scipy CSR of the block matrix, explicit zeros kept (the product that makes the "cancel" loads)"""
    import scipy.sparse as sp

    rowptr, colidx, vals = _bsr(K)
    n = len(rowptr) - 1
    return sp.bsr_matrix((vals, colidx, rowptr), shape=(6 * n, 6 * n)).tocsr()


def states(K, F, free, seed=5):
    """{state: (x, F of that state)}: x random on the free dofs, zero on the others"""
    M = csr(K)
    F = np.asarray(F, dtype=np.float64).reshape(-1)
    x = np.random.default_rng(seed).normal(size=len(F)) * free
    Kx = M @ x
    return {"cancel": (x, Kx), "zero": (x, np.zeros_like(F)), "free": (x * (np.linalg.norm(F) / np.linalg.norm(Kx)), F)}


def cancellation(truth, S):
    """how far a state cancels: ||r*|| / ||S||"""
    return float(np.linalg.norm(truth) / np.linalg.norm(S))
