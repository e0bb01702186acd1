"""Truth, restatement and inputs for the dense inverse of the coarsest multigrid operator (csrc/amg_dense.hip, and the host's
Cholesky path csrc/amg_setup.cpp dense_inverse).  Pure numpy: runs anywhere.

truth_inverse     long-double Cholesky inverse (x87 extended: 64-bit significand), with one long-double Newton step where asked
restated_inverse  the device's method in plain double: scalar symmetric sweeps, IEEE division, the project's two pivot rules
err               max|X - X*| / max|X*|
families          (a) random SPD, (b) graded and shell-like, (c) Galerkin operators of the host coarsening, (d) planted dead
                  directions, (e) the planted pivot either side of the drop threshold, (f) clear failures -- all as block CSR
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
DROP = 1e-11      # a pivot at or below DROP x its original diagonal entry is dropped (zero row and column of the inverse)
FAIL = 1e-4       # a pivot below -FAIL x |its original diagonal entry|, or an original entry that is not positive: breakdown
SWEEP = 128       # csrc/amg_dense.hip kSW: the matrix is padded to a multiple of it
TILE = 64         # kNB
BREAKDOWN = -5    # include/femshell.h FEMSHELL_ERR_BREAKDOWN


def n_pad(n):
    return (n + SWEEP - 1) // SWEEP * SWEEP


# ---- truth -------------------------------------------------------------------------------------------------------------------
def _cholesky_ld(A):
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for c in range(n):
        v = A[c:, c] - L[c:, :c] @ L[c, :c]
        assert v[0] > 0, "truth_inverse: not positive definite at %d" % c
        d = np.sqrt(v[0])
        L[c, c] = d
        L[c + 1:, c] = v[1:] / d
    return L


def _lower_inverse_ld(L):
    n = L.shape[0]
    Y = np.zeros((n, n), dtype=LD)
    for r in range(n):
        Y[r, :r] = -(L[r, :r] @ Y[:r, :r]) / L[r, r]
        Y[r, r] = 1 / L[r, r]
    return Y


def _gram_of_lower_ld(Y, nb=128):
    """Y^T Y of a lower-triangular Y, block by block over the non-zero part only"""
    n = Y.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, nb):
        i1 = min(n, i0 + nb)
        for j0 in range(0, i0 + 1, nb):
            j1 = min(n, j0 + nb)
            X[i0:i1, j0:j1] = Y[i0:, i0:i1].T @ Y[i0:, j0:j1]
            if j0 != i0:
                X[j0:j1, i0:i1] = X[i0:i1, j0:j1].T
    return X


def defect(A, X):
    """max|A X - I| in long double"""
    R = np.asarray(A, dtype=LD) @ np.asarray(X, dtype=LD)
    R[np.diag_indices_from(R)] -= 1
    return float(np.abs(R).max())


def truth_inverse(A, need=None, info=None):
    """Long-double Cholesky inverse of a symmetric positive definite A (a double array).

    need: the error (in the metric `err`) of the double paths this truth is to judge.  The truth's own error is estimated by
    the Newton correction X (A X - I) it would get; where that is not 100 x below `need`, the correction is applied (one
    long-double Newton step X (2 I - A X)).  info (a dict) receives the long-double defect max|A X - I| and that estimate."""
    Al = np.asarray(A, dtype=LD)
    X = _gram_of_lower_ld(_lower_inverse_ld(_cholesky_ld(Al)))
    X = 0.5 * (X + X.T)
    if need is not None or info is not None:
        R = Al @ X
        R[np.diag_indices_from(R)] -= 1
        own = float(np.abs(X.astype(np.float64) @ R.astype(np.float64)).max() / np.abs(X).max())  # (an estimate: double is enough)
        if info is not None:
            info.update(defect=float(np.abs(R).max()), own_error=own, newton=False)
        if need is not None and not own * 100.0 <= need:
            X = X - X @ R
            X = 0.5 * (X + X.T)
            if info is not None:
                info.update(newton=True, defect=defect(Al, X))
    return X


def embedded_truth(A, dead, need=None, info=None):
    """the inverse of A without the rows and columns `dead`, embedded with zero rows and columns"""
    n = A.shape[0]
    keep = np.setdiff1d(np.arange(n), np.asarray(sorted(dead), dtype=np.int64))
    X = np.zeros((n, n), dtype=LD)
    X[np.ix_(keep, keep)] = truth_inverse(A[np.ix_(keep, keep)], need=need, info=info)
    return X


def err(X, truth):
    T = np.asarray(truth, dtype=LD)
    return float(np.abs(np.asarray(X, dtype=LD) - T).max() / np.abs(T).max())


def bound(restated_err, n, factor=4.0):
    """What the device's block method may be off by: `factor` (tests/helpers/truth.py bound: two bits) times the error of the
    same method restated in plain double on the same matrix, and never below n 2^-53 (n roundings of a unit-sized sum)"""
    return factor * max(restated_err, n * U)


# ---- the method, restated ----------------------------------------------------------------------------------------------------
def restated_inverse(A):
    """Symmetric sweep operator (Goodnight 1979) one scalar pivot at a time in IEEE double, pivots tested against the ORIGINAL
    diagonal: returns (inverse, dropped indices, None), or (None, dropped so far, failing index)."""
    try:
        from scipy.linalg.blas import dger
    except ImportError:  # pragma: no cover
        dger = None
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    M = np.asfortranarray(np.tril(A) + np.tril(A, -1).T)  # the lower triangle is the matrix (the device reads nothing else)
    a0 = np.diag(M).copy()
    dropped = []
    for k in range(n):
        d, a = M[k, k], a0[k]
        if not (a > 0.0) or d < -FAIL * abs(a):
            return None, dropped, k
        col = M[:, k].copy()
        if d <= DROP * a:
            dropped.append(k)
            M[:, k] = 0.0
            M[k, :] = 0.0
            continue
        inv = 1.0 / d
        col[k] = 0.0
        if dger is not None:
            M = dger(-inv, col, col, a=M, overwrite_a=1)
        else:
            M -= np.outer(col * inv, col)
        M[:, k] = col * inv
        M[k, :] = col * inv
        M[k, k] = -inv
    X = -M
    return np.ascontiguousarray(0.5 * (X + X.T)), dropped, None


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def to_block_csr(A):
    """a dense (6 m) x (6 m) matrix as block CSR with every block stored: (rowptr int32, colidx int32, vals [m*m, 6, 6])"""
    n = A.shape[0]
    assert n % 6 == 0
    m = n // 6
    rowptr = (np.arange(m + 1) * m).astype(np.int32)
    colidx = np.tile(np.arange(m, dtype=np.int32), m)
    vals = np.ascontiguousarray(A.reshape(m, 6, m, 6).transpose(0, 2, 1, 3)).reshape(m * m, 6, 6)
    return rowptr, colidx, vals


def from_block_csr(rowptr, colidx, vals):
    m = len(rowptr) - 1
    A = np.zeros((m, 6, m, 6))
    vals = np.asarray(vals).reshape(-1, 6, 6)
    for i in range(m):
        for q in range(rowptr[i], rowptr[i + 1]):
            A[i, :, colidx[q], :] = vals[q]
    return A.reshape(6 * m, 6 * m)


def _orthogonal(n, rng):
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(R))


def _sym(A):
    return 0.5 * (A + A.T)


def random_spd(nodes, seed=0):
    """(a) random SPD, condition number 1e2: a layout mistake shows at 1e-14 here"""
    n = 6 * nodes
    rng = np.random.default_rng(1000 + 7 * nodes + seed)
    Q = _orthogonal(n, rng)
    lam = np.logspace(0.0, 2.0, n) if n > 1 else np.ones(1)
    return _sym((Q * lam) @ Q.T)


def graded(nodes, decades=6.5, seed=0):
    """(b) graded and shell-like: a spectrum over `decades` decades, rotational dofs scaled x30 against the translations (the
    diagonal entries then differ by 1e3 and the pivot test against the ORIGINAL diagonal entry matters)"""
    n = 6 * nodes
    rng = np.random.default_rng(2000 + 7 * nodes + seed)
    Q = _orthogonal(n, rng)
    lam = np.logspace(0.0, decades, n)
    s = np.tile(np.array([1.0, 1.0, 1.0, 30.0, 30.0, 30.0]), nodes)
    return _sym(((Q * lam) @ Q.T) * s[:, None] * s[None, :])


def planted(nodes, dead, seed=0):
    """(d) M = G G^T with small integer G (exact in double); every row p in `dead` of G is an integer combination of rows with
    smaller index, so the pivot at p is 0 in exact arithmetic and nothing else depends on it"""
    n = 6 * nodes
    rng = np.random.default_rng(3000 + 7 * nodes + seed)
    G = rng.integers(-2, 3, size=(n, 2 * n)).astype(np.float64)
    for p in sorted(dead):
        assert 2 <= p < n
        src = rng.choice(p, size=2, replace=False)
        src = [s for s in src if s not in dead] or [0]
        G[p] = sum((1.0 if k % 2 == 0 else -1.0) * G[s] for k, s in enumerate(src))
    A = G @ G.T
    assert np.all(A == np.rint(A)) and np.abs(A).max() < 2.0 ** 40
    return A


def near_threshold(nodes, p, rel, seed=0):
    """(e) the planted matrix with A[p,p] raised by `rel` of itself: the pivot at p is rel x its diagonal entry"""
    A = planted(nodes, [p], seed)
    A[p, p] *= 1.0 + rel
    return A


def clearly_negative(nodes, p, seed=0):
    """(f) the planted matrix with A[p,p] halved: the pivot at p is -1 x its diagonal entry"""
    A = planted(nodes, [p], seed)
    A[p, p] *= 0.5
    return A


def zero_diagonal(nodes, q, seed=0):
    """(f) a family (a) matrix with one zero diagonal entry"""
    A = random_spd(nodes, seed)
    A[q, q] = 0.0
    return A


def galerkin(kind):
    """(c) the coarse operator of one step of the host coarsening on a small mesh: (rowptr, colidx, vals) as the library made them"""
    import importlib

    from tests.helpers import meshes, oracle

    binding = importlib.import_module("fem-shell_amd.binding")
    if kind == "panel":
        m = meshes.structured(24, 20, 0, 0, 6, 5, kind="t", ul_lr=True, bcids=(0, 0, 1, -1), factor=300.0, loading=2)
        mat = oracle.material(0.3, 1e7, 0.5)
    else:
        m = meshes.scordelis_lo(18)
        mat = oracle.material(*m.material)
    dm = m.dirichlet_mask()
    rp, ci, vals, _ = oracle.assemble(m.xyz, m.tri, m.quad, mat, dm, m.loads)
    h = binding.amg_host_coarsen(rp, ci, vals, binding.amg_host_rbm(m.xyz, dm), 2.5)
    return h["Ac_rowptr"].astype(np.int32), h["Ac_cols"].astype(np.int32), h["Ac_vals"]


# ---- the tile map of the trailing update -------------------------------------------------------------------------------------
SB = 8  # tiles per side of a super-block


def tile_map_model(nt):
    """numpy model of dense_tile_map_lists (csrc/amg_setup.cpp): super-blocks sorted by weight (stable), each dealt to the least
    loaded of eight lists (first of equals), lists in row-major order: [8, per_xcd] of (I << 16) | J, -1 = none"""
    nsbr = (nt + SB - 1) // SB
    sbs = []
    for I in range(nsbr):
        for J in range(I + 1):
            w = sum(1 for a in range(SB) for b in range(SB) if SB * I + a < nt and SB * J + b <= SB * I + a)
            sbs.append((I, J, w))
    sbs.sort(key=lambda s: -s[2])  # (stable)
    lists, load = [[] for _ in range(8)], [0] * 8
    for I, J, w in sbs:
        x = load.index(min(load))
        lists[x].append((I, J))
        load[x] += w
    per = max(1, max(len(l) for l in lists))
    out = np.full((8, per), -1, dtype=np.int32)
    for x in range(8):
        for k, (I, J) in enumerate(sorted(lists[x])):
            out[x, k] = (I << 16) | J
    return out


def tiles_of_map(lists, nt):
    """how often the workgroups of k_dense_update (no look-ahead) reach each tile: counts[i, j], by the kernel's own index arithmetic"""
    per = lists.shape[1]
    counts = np.zeros((nt, nt), dtype=np.int64)
    for m in range(8 * per * SB * SB):
        idx = m >> 3
        sb = int(lists[m & 7, idx // (SB * SB)])
        tin = idx % (SB * SB)
        if sb < 0:
            continue
        i, j = SB * (sb >> 16) + tin // SB, SB * (sb & 0xFFFF) + tin % SB
        if i >= nt or j > i:
            continue
        counts[i, j] += 1
    return counts


# ---- the cases of tests/test_gpu_dense_inverse.py and tools/dense_inverse_report.py ------------------------------------------
# nodes (n = 6 nodes): the smallest sizes at which each mechanism of csrc/amg_dense.hip first exists
#   1: almost all padding, one sweep            11: the Schur half of the only pivot block holds 2 live rows
#  21: one sweep, 2 padding rows                22: two sweeps, 124 padding rows, first use of the look-ahead
#  32: the last 64-tile entirely padding        64: n = 384, an exact multiple of 128 (no padding rows)
#  86: nt = 10, a second super-block row       128: n = 768, exact multiple again, nt = 12
# 171: nt = 18, three super-block rows (family (b) only: the truth takes seconds there)
SHAPES = (1, 11, 21, 22, 32, 64, 86, 128, 171)
VARIANT_SHAPES = (22, 86, 171)
ACCURACY_CASES = [("a", s) for s in SHAPES if s != 171] + [("b", s) for s in SHAPES] + [("c", "panel"), ("c", "roof")]
# planted dead directions at n_pad = 256 (40 nodes, n = 240) and 384 (43 nodes, n = 258): in the first 64 of a pivot block (B_A),
# in the second 64 (B_S), two in one group of four pivots, in pivot block K >= 1 (computed on the look-ahead's stream), and the
# last live row before the padding
PLANTED_CASES = [(40, (20,)), (40, (70,)), (40, (5, 6)), (40, (130,)), (40, (200,)), (40, (198, 199)), (40, (239,)),
                 (43, (70,)), (43, (5, 6)), (43, (130, 200)), (43, (257,)), (43, (256, 257))]

_cache = {}


def case(fam, which):
    """One accuracy case, computed once per process: the matrix as block CSR and dense, its truth, the errors of the restatement
    and of LAPACK against it, the condition number.  ("d", (nodes, dead)): a planted matrix and its embedded truth."""
    key = (fam, which)
    if key in _cache:
        return _cache[key]
    if fam == "c":
        bcsr = galerkin(which)
        A = from_block_csr(*bcsr)
        A = np.tril(A) + np.tril(A, -1).T  # what the device reads: the lower triangle
    elif fam == "d":
        A = planted(which[0], which[1])
        bcsr = to_block_csr(A)
    else:
        A = (random_spd if fam == "a" else graded)(which)
        bcsr = to_block_csr(A)
    dead = list(which[1]) if fam == "d" else []
    R, dropped, failed = restated_inverse(A)
    assert failed is None and dropped == sorted(dead)
    keep = np.setdiff1d(np.arange(len(A)), dead)
    Ak = A[np.ix_(keep, keep)]
    lap = np.zeros_like(A)
    lap[np.ix_(keep, keep)] = np.linalg.inv(Ak)
    rough = float(np.abs(R - lap).max() / np.abs(lap).max())
    info = {}
    X = embedded_truth(A, dead, need=rough, info=info)
    c = dict(fam=fam, which=which, A=A, bcsr=bcsr, n=len(A), dead=dead, truth=X, truth_info=info, restated=R, e_restated=err(R, X),
             e_lapack=err(lap, X), cond=float(np.linalg.cond(Ak)))
    Xb, b_dead, b_failed = restated_block_inverse(A)
    assert b_dead == len(dead) and b_failed == 0
    c["e_block"] = err(Xb, X)
    c["kappa_pivot"] = pivot_block_condition(A, lap) if not dead else float("nan")
    # Families (a), (c), (d): the standing bound, 4 x the scalar restatement.  Family (b), graded over six decades: the explicitly
    # formed inverses of the pivot blocks cost cond(pivot block) u ("What the dense inverse is held to"), which
    # the scalar sweep never pays; the device is held to 4 x what its own arithmetic restated in plain double shows
    # (restated_block_inverse) or, where that one realisation happens to be lucky, what one rounding in the inverse of the
    # worst-conditioned pivot block costs.
    allowed = c["e_restated"] if fam != "b" else max(c["e_restated"], c["e_block"], c["kappa_pivot"] * U)
    c["bound"] = bound(allowed, c["n"])
    _cache[key] = c
    return c


def pivot_block_condition(A, inverse):
    """the largest 2-norm condition number among the 128 x 128 pivot blocks as the block sweep meets them (the leading block of the
    Schur complement of everything swept before: the inverse of the trailing part of A^-1), live rows only.  Every inverse the
    method forms explicitly is that of a principal submatrix of such a block or of a Schur complement inside it: none is worse."""
    n = len(A)
    worst = 0.0
    for k0 in range(0, n, SWEEP):
        P = (A if k0 == 0 else np.linalg.inv(inverse[k0:, k0:]))[:SWEEP, :SWEEP]
        worst = max(worst, float(np.linalg.cond(0.5 * (P + P.T))))
    return worst


# ---- the method restated at its block structure ------------------------------------------------------------------------------
# csrc/amg_dense.hip does not sweep one scalar pivot at a time: it forms the inverse of a pivot block EXPLICITLY at three nested
# levels and multiplies with it -- groups of four pivots inside a 64 x 64 register sweep (sweep64), the two 64-halves of a pivot
# block joined through their Schur complement (pivot_block), and the 128-wide block sweep itself (W = C B, A -= W C^T).  A product
# with an explicitly formed inverse of a block P carries cond(P) u where sequential elimination carries u; the model below is that
# arithmetic in plain double (numpy products in place of the matrix cores', IEEE division in place of rcp + two Newton steps).
def _sweep4(m, a0, state):
    """scalar symmetric sweeps of a 4 x 4 pivot sub-block against the original diagonal entries a0: m <- -(m^-1) on the live directions"""
    for k in range(4):
        d, a = m[k, k], a0[k]
        failed = not (a > 0.0) or d < -FAIL * abs(a)
        dead = failed or d <= DROP * a
        state["failed"] += int(failed)
        state["dead"] += int(dead)
        inv = 0.0 if dead else 1.0 / d
        col = m[:, k].copy()
        others = [i for i in range(4) if i != k]
        for i in others:
            for j in others:
                m[i, j] -= col[i] * col[j] * inv
        for i in others:
            m[i, k] = m[k, i] = col[i] * inv
        m[k, k] = -inv


def _sweep64_model(S, a0, state):
    """sweep64: four pivots at a time, the rank-4 update with the explicitly swept 4 x 4 block: returns -(S^-1) on the live directions"""
    S = S.copy()
    n = len(S)
    for g in range(0, n, 4):
        grp = np.arange(g, g + 4)
        rest = np.concatenate([np.arange(0, g), np.arange(g + 4, n)])
        R = S[grp, :].copy()
        m = R[:, grp].copy()
        _sweep4(m, a0[g:g + 4], state)
        T = -(R[:, rest].T @ m)                   # ti = -R_i^T m
        S[np.ix_(rest, rest)] -= T @ R[:, rest]   # S_ij <- S_ij - ti R_j
        S[np.ix_(rest, grp)] = T
        S[np.ix_(grp, rest)] = T.T
        S[np.ix_(grp, grp)] = m
    return S


def _pivot_block_model(P, a0, state):
    """pivot_block: B = P^-1 (128 x 128) from the two 64 x 64 sweeps and four products"""
    A, C, D = P[:64, :64], P[64:, :64], P[64:, 64:]
    BA = -_sweep64_model(A, a0[:64], state)
    W = C @ BA
    Sc = D - W @ C.T
    Sc = np.tril(Sc) + np.tril(Sc, -1).T
    BS = -_sweep64_model(Sc, a0[64:], state)
    X21 = -(BS @ W)
    B = np.empty((128, 128))
    B[:64, :64] = BA - W.T @ X21
    B[64:, :64] = X21
    B[:64, 64:] = X21.T
    B[64:, 64:] = BS
    return B


def restated_block_inverse(A):
    """The device's arithmetic in plain double (see above): (inverse, number of dropped directions, number of failed pivots)."""
    A = np.asarray(A, dtype=np.float64)
    n = len(A)
    npad = n_pad(n)
    M = np.eye(npad)
    M[:n, :n] = np.tril(A) + np.tril(A, -1).T
    a0 = np.diag(M).copy()
    state = {"dead": 0, "failed": 0}
    for k0 in range(0, npad, SWEEP):
        K = np.arange(k0, k0 + SWEEP)
        Rr = np.concatenate([np.arange(0, k0), np.arange(k0 + SWEEP, npad)])
        B = _pivot_block_model(M[np.ix_(K, K)], a0[K], state)
        C = M[np.ix_(Rr, K)]
        W = C @ B
        M[np.ix_(Rr, Rr)] -= W @ C.T
        M[np.ix_(Rr, K)] = W
        M[np.ix_(K, Rr)] = W.T
        M[np.ix_(K, K)] = -B
    X = -M[:n, :n]
    X = np.tril(X) + np.tril(X, -1).T  # (the device keeps the lower triangle)
    return X, state["dead"], state["failed"]
