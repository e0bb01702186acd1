"""The 6 x 6 block-Jacobi inverse (csrc/kernels.hip k_block_jacobi, csrc/amg_setup.cpp spd_inverse6, oracle/amg_oracle.py
block_diag_inverse) and the spectral bound of a multigrid level (power_iteration_start / _finish, on one rank and on a row partition) against
truths that owe nothing to either: pure numpy, runs anywhere.

truth(A)      the exact inverse of a 6 x 6 matrix of doubles in rational arithmetic, rounded once to long double -- exact, so there
              is no question of the truth's own error on a block of condition 1e12
restated(A)   the kernel's method in plain double, statement by statement
err(B, T, A)  max|S (B - T) S| / max|S T S|, S = diag(sqrt(A_ii)).  Cholesky is invariant under a diagonal scaling (the scaled
              problem is the same computation up to the roundings of the scaling itself), and a shell block is badly scaled by
              nature -- translations E t, rotations E t^3, the drilling penalty far below: the raw max-norm would only see the
              softest entries of the inverse
bound         the project's standing one (tests/helpers/truth.py bound): a family's worst error may be 4 x the restatement's
              worst over the same family, and never needs to be below 16 eps.  No number of it comes from the device.
"""
from fractions import Fraction

import numpy as np

from tests.helpers import truth as element_truth

LD = np.longdouble
EPS = 2.0 ** -52
_LD_BITS = np.finfo(LD).nmant + 1  # 64 on x86 (the explicit leading bit counts), 53 where long double is double
PER_FAMILY = 256


# ---- the truth -----------------------------------------------------------------------------------------------------------------
def _round_fraction(f):
    """the long double nearest to a Fraction (ties to even)"""
    if f == 0:
        return LD(0)
    sign = -1 if f < 0 else 1
    p, q = abs(f.numerator), f.denominator
    s = _LD_BITS - (p.bit_length() - q.bit_length())  # p 2^s / q lies in (2^(bits-1), 2^(bits+1))
    num, den = (p << s, q) if s >= 0 else (p, q << -s)
    if num // den >= 1 << _LD_BITS:
        s -= 1
        num, den = (p << s, q) if s >= 0 else (p, q << -s)
    m, rem = divmod(num, den)
    if 2 * rem > den or (2 * rem == den and (m & 1)):
        m += 1
    # (m has up to 64 bits: in two exact halves)
    v = np.ldexp(LD(m >> 32), 32) + LD(m & 0xFFFFFFFF)
    return sign * np.ldexp(v, -s)


def _exact_inverse(A):
    """Gauss-Jordan with exact pivots (any non-zero one) on Fractions: list of rows, or None for a singular matrix"""
    n = len(A)
    M = [[Fraction(float(A[i][j])) for j in range(n)] + [Fraction(int(i == j)) for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c] != 0), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        inv = 1 / M[c][c]
        M[c] = [v * inv for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


_truths = {}


def truth(A):
    """The inverse of the 6 x 6 doubles A as long doubles, each entry the exact value rounded once.  Cached per process."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    assert A.shape == (6, 6) and np.isfinite(A).all()
    key = A.tobytes()
    if key not in _truths:
        X = _exact_inverse(A)
        assert X is not None, "singular block"
        _truths[key] = np.array([[_round_fraction(v) for v in row] for row in X], dtype=LD)
    return _truths[key]


def truths(blocks):
    return np.array([truth(b) for b in np.asarray(blocks).reshape(-1, 6, 6)], dtype=LD).reshape(-1, 6, 6)


# ---- the method, restated --------------------------------------------------------------------------------------------------------
def restated(A, divide=False):
    """k_block_jacobi in plain IEEE double on blocks A [..., 6, 6], statement by statement (every array operation below is one
    rounded scalar operation per block): Cholesky with il = 1 / sqrt(d) and v * il, Li by forward substitution, B = Li^T Li on the
    upper triangle, mirrored; a pivot that is not > 0 (NaN included) makes the block's result the identity.  Reads the diagonal
    and the strict LOWER triangle's mirror image, as the kernel does under diag_upper: A[r][c], r > c, is taken from A[c][r].
    divide: the host's rounding variant (spd_inverse6: v / lcc instead of v * il).  Returns (B [..., 6, 6], ok [...])."""
    A = np.asarray(A, dtype=np.float64)
    lead = A.shape[:-2]
    A = A.reshape(-1, 6, 6)
    m = len(A)
    L = np.zeros((m, 6, 6))
    Li = np.zeros((m, 6, 6))
    ok = np.ones(m, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(6):
            d = A[:, c, c].copy()
            for k in range(c):
                d = d - L[:, c, k] * L[:, c, k]
            bad = ~(d > 0.0)
            ok &= ~bad
            d = np.where(bad, 1.0, d)
            lcc = np.sqrt(d)
            il = 1.0 / lcc
            L[:, c, c] = lcc
            for r in range(c + 1, 6):
                v = A[:, c, r].copy()
                for k in range(c):
                    v = v - L[:, r, k] * L[:, c, k]
                L[:, r, c] = v / lcc if divide else v * il
        for c in range(6):
            Li[:, c, c] = 1.0 / L[:, c, c]
            for r in range(c + 1, 6):
                v = np.zeros(m)
                for k in range(c, r):
                    v = v - L[:, r, k] * Li[:, k, c]
                Li[:, r, c] = v / L[:, r, r]
        B = np.zeros((m, 6, 6))
        for i in range(6):
            for j in range(i, 6):
                v = np.zeros(m)
                for k in range(j, 6):
                    v = v + Li[:, k, i] * Li[:, k, j]
                B[:, i, j] = v
                B[:, j, i] = v
    B[~ok] = np.eye(6)
    return B.reshape(lead + (6, 6)), ok.reshape(lead)


# ---- the metric and the bound ----------------------------------------------------------------------------------------------------
def err(B, T, A):
    """max|S (B - T) S| / max|S T S| with S = diag(sqrt(A_ii)), in long double; B, T, A [..., 6, 6] -> [...]"""
    B, T, A = (np.asarray(x) for x in (B, T, A))
    s = np.sqrt(np.diagonal(A, axis1=-2, axis2=-1).astype(LD))
    S = s[..., :, None] * s[..., None, :]
    T = T.astype(LD)
    return (np.abs((B.astype(LD) - T) * S).max(axis=(-2, -1)) / np.abs(T * S).max(axis=(-2, -1))).astype(np.float64)


def worst(B, T, A):
    return float(np.max(err(B, T, A)))


def bound(restated_worst, factor=4.0):
    return element_truth.bound(restated_worst, factor)


def scaled_condition(A):
    s = np.sqrt(np.diag(A))
    w = np.linalg.eigvalsh(A / np.outer(s, s))
    return float(w[-1] / w[0])


# ---- block families -----------------------------------------------------------------------------------------------------------------
def _orthogonal(rng):
    Q, R = np.linalg.qr(rng.standard_normal((6, 6)))
    return Q * np.sign(np.diag(R))


def _spd(rng, decades):
    Q = _orthogonal(rng)
    A = (Q * np.logspace(0.0, decades, 6)) @ Q.T
    return 0.5 * (A + A.T)


SHELL_SCALE = np.array([1.0, 1.0, 1.0, 1e-4, 1e-4, 1e-6])
SYNTHETIC = ("random", "shell", "graded6", "graded9", "graded12")
# the restatement's worst error over the 256 blocks of a family, as first measured on the CPU: tests/test_jacobi_truth_cpu.py holds
# what restated() gives today inside a factor of two of these, so that the bound of the device's tests cannot drift
RESTATED_WORST = {"random": 6.3e-15, "shell": 6.0e-14, "graded6": 5.0e-11, "graded9": 3.2e-8, "graded12": 3.2e-5}

_families = {}


def family(name, count=PER_FAMILY):
    """[count, 6, 6] SPD blocks: random (condition 1e2) / shell (a condition-1e3 block under the diagonal scaling of a shell
    node, translations 1, rotations 1e-4, drilling 1e-6, each times 10^U(-2, 2): raw condition up to 1e15, scaled 1e3) / graded6,
    graded9, graded12 (spectrum over that many decades)"""
    key = (name, count)
    if key not in _families:
        # (graded12: the worst of 256 blocks at condition 1e12 moves by a factor of two with the seed -- 15, 25, 35, 45, 55 give 1.82,
        #  1.30, 1.34, 1.11, 2.03 x the 3.2e-5 recorded in RESTATED_WORST; 45 sits in the middle of the pin of
        #  tests/test_jacobi_truth_cpu.py instead of at its edge.  The choice looks at the CPU restatement only.)
        rng = np.random.default_rng({"random": 11, "shell": 12, "graded6": 13, "graded9": 14, "graded12": 45}[name])
        out = np.zeros((count, 6, 6))
        for k in range(count):
            if name == "random":
                out[k] = _spd(rng, 2.0)
            elif name == "shell":
                d = np.sqrt(SHELL_SCALE * 10.0 ** rng.uniform(-2.0, 2.0, 6))
                C = _spd(rng, 3.0)
                out[k] = np.triu(C * d[:, None] * d[None, :])
                out[k] = out[k] + np.triu(out[k], 1).T  # (exactly symmetric)
            else:
                out[k] = _spd(rng, float(name[6:]))
        out.setflags(write=False)
        _families[key] = out
    return _families[key]


_cases = {}


def case(name):
    """dict of a synthetic family: blocks A, truth T, restated B with its errors and worst, the bound of the device and the host"""
    if name not in _cases:
        A = family(name)
        T = truths(A)
        B, ok = restated(A)
        assert ok.all()
        e = err(B, T, A)
        _cases[name] = {"A": A, "T": T, "B": B, "e_restated": e, "worst": float(e.max()), "bound": bound(float(e.max()))}
    return _cases[name]


def failures():
    """Family (f): [(label, block)] -- a first non-positive pivot planted at each of the six positions (zero, and negative), an
    all-zero block, one NaN entry (on the diagonal, and above it).  restated() returns (identity, False) for every one."""
    rng = np.random.default_rng(16)
    out = []
    for p in range(6):
        for kind in ("zero", "negative"):
            # G lower triangular with unit-sized integer entries: A = G J G^T is exact in double, its Cholesky pivots are those of J
            G = np.tril(rng.integers(-2, 3, size=(6, 6))).astype(np.float64)
            G[np.arange(6), np.arange(6)] = rng.integers(1, 4, size=6)
            J = np.ones(6)
            J[p] = 0.0 if kind == "zero" else -1.0
            out.append(("pivot%d-%s" % (p, kind), (G * J) @ G.T))
    out.append(("all-zero", np.zeros((6, 6))))
    for (i, j) in ((2, 2), (1, 4)):
        A = _spd(rng, 2.0)
        A[i, j] = A[j, i] = np.nan
        out.append(("nan%d%d" % (i, j), A))
    return out


# ---- launches: blocks on the diagonal of a block CSR matrix ----------------------------------------------------------------------------
NODE_COUNTS = (1, 31, 32, 33, 65, 256)  # a lone node, a last slice of one node short, exactly one slice, one node over, several slices


def launch_matrix(diag_blocks, seed=0, poison_lower=False):
    """(rowptr, colidx, vals) of a symmetric block matrix with the given diagonal blocks and, per node, a few off-diagonal blocks
    with columns below and above the diagonal (large entries: a reader that took another slot for the diagonal one would show).
    poison_lower: NaN in the strict lower triangle of every diagonal block."""
    D = np.asarray(diag_blocks, dtype=np.float64).reshape(-1, 6, 6)
    n = len(D)
    rng = np.random.default_rng(500 + n + seed)
    pairs = set()
    for a in range(n):
        for off in (1, 3, 7):
            if a + off < n and (off == 1 or rng.random() < 0.6):
                pairs.add((a, a + off))
    blocks = {(a, a): D[a].copy() for a in range(n)}
    for (a, b) in pairs:
        M = 1e3 * rng.standard_normal((6, 6))
        blocks[(a, b)] = M
        blocks[(b, a)] = M.T.copy()
    if poison_lower:
        for a in range(n):
            blocks[(a, a)][np.tril_indices(6, -1)] = np.nan
    keys = sorted(blocks)
    rowptr = np.zeros(n + 1, dtype=np.int32)
    for (a, _) in keys:
        rowptr[a + 1] += 1
    rowptr = np.cumsum(rowptr).astype(np.int32)
    colidx = np.array([b for (_, b) in keys], dtype=np.int32)
    vals = np.array([blocks[k] for k in keys]).reshape(-1, 6, 6)
    return rowptr, colidx, vals


def diagonal_blocks(rowptr, colidx, vals):
    """the diagonal blocks [n, 6, 6] of a block CSR matrix (every row has one)"""
    rowptr, colidx = np.asarray(rowptr), np.asarray(colidx)
    vals = np.asarray(vals).reshape(-1, 6, 6)
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    q = np.flatnonzero(colidx == rows)
    assert len(q) == n and np.array_equal(rows[q], np.arange(n))
    return vals[q]


# ---- real blocks: K on the element families of tests/golden/element_truth.npz ----------------------------------------------------------
# Dirichlet masks dealt out to the nodes in turn: none, some, all six dofs constrained (a constrained dof carries its valence --
# the number of elements at the node -- on the diagonal and zeros beside it)
MASKS = (0, 0, 0b000111, 0, 0b101010, 0b100000, 0b111111, 0, 0b011111)


def real_cases():
    """[(label, flags, sections.Case)]: per family of the fixture and per value of its elements' flags one mesh of isolated
    elements (tests/helpers/truth.py isolated_mesh, in as many copies as give 40 nodes: more than one slice), every element with its own material as a
    section, and the masks above.  Slivers, far-away quadrilaterals, t = 1e-5 and nu near 0.5 are among them."""
    from tests.helpers import sections

    fx = element_truth.load()
    out = []
    for fam in element_truth.FAMILIES:
        tri_fam = element_truth.nodes_of(fam) == 3
        for key, els in element_truth.groups_of(fx, fam, None, own=True).items():
            flags = int(key[3])
            X = [fx[fam + "_xyz"][e] for e in els]
            table, index = element_truth.section_table([element_truth.material_of(fx, fam, e)[:3] for e in els])
            reps = max(2, -(-40 // (len(X) * element_truth.nodes_of(fam))))
            xyz, tri, quad = element_truth.isolated_mesh(X if tri_fam else None, None if tri_fam else X, reps)
            idx = np.tile(index, reps)
            dmask = np.array([MASKS[(a + len(out)) % len(MASKS)] for a in range(len(xyz))], dtype=np.uint8)
            out.append(("%s-flags%d" % (fam, flags), flags,
                        sections.Case(xyz, tri, quad, table, idx if tri_fam else None, None if tri_fam else idx, dmask,
                                      np.zeros((len(xyz), 6)))))
    return out


def as_read(blocks, upper):
    """the symmetric blocks k_block_jacobi works on: the diagonal and the upper triangle mirrored (DeviceMatrix::diag_upper, K
    under symmetric storage), or the diagonal and the lower triangle mirrored (whole blocks: its Cholesky reads A[r][c], r > c)"""
    blocks = np.asarray(blocks, dtype=np.float64).reshape(-1, 6, 6)
    T = np.triu(blocks) if upper else np.tril(blocks)
    return T + np.swapaxes(np.triu(T, 1) if upper else np.tril(T, -1), -1, -2)


# ---- the meshes of the spectral-bound tests (their coarse operators are family (e) of the block-inverse tests) -------------------
SPECTRAL_MESHES = ("curved", "panel", "cylinder", "strip", "quads", "delaunay")


def spectral_mesh(name):
    """(xyz, tri, quad, dmask, loads, (nu, E, t)) of a mesh of 250 to 600 nodes"""
    from tests.helpers import meshes, sections

    if name == "curved":
        m = sections.curved_patch(24, 18)
        mat = (0.3, 2e5, 0.05)
    elif name == "panel":  # the panel of tests/helpers/dense_truth.py galerkin
        m = meshes.structured(24, 20, 0, 0, 6, 5, kind="t", ul_lr=True, bcids=(0, 0, 1, -1), factor=300.0, loading=2)
        mat = (0.3, 1e7, 0.5)
    elif name == "cylinder":
        m = meshes.pinched_cylinder(20, 20)
        mat = tuple(m.material)
    elif name == "strip":  # clamped all round: a third of the nodes Dirichlet
        m = meshes.structured(40, 6, 0, 0, 16.0, 1.0, kind="t", ul_lr=True, bcids=(1, 1, 1, 1), factor=300.0, loading=2)
        mat = (0.3, 1e7, 0.05)
    elif name == "quads":
        m = meshes.structured(16, 16, 0, 0, 10, 10, kind="q", bcids=(1, 1, 1, 1), factor=300.0, loading=2)
        mat = (0.3, 1e7, 0.5)
    elif name == "delaunay":
        xyz, tri = meshes.delaunay_patch(600, 2)
        dmask = np.zeros(len(xyz), dtype=np.uint8)
        dmask[xyz[:, 0] < 0.2] = 0x3F
        return xyz, tri, None, dmask, np.random.default_rng(3).normal(size=(len(xyz), 6)), (0.3, 7.0e4, 0.03)
    else:
        raise ValueError(name)
    tri = m.tri if m.tri is not None and len(m.tri) else None
    quad = m.quad if m.quad is not None and len(m.quad) else None
    return m.xyz, tri, quad, m.dirichlet_mask(), m.loads, mat


def spectral_context(pkg, name, flags=None, coarsest_nodes=60):
    """a multigrid context of one of those meshes, assembled (the hierarchy is built by the first call that needs it)"""
    xyz, tri, quad, dmask, loads, mat = spectral_mesh(name)
    fs = pkg.FemShell(*mat, device=0) if flags is None else pkg.FemShell(*mat, flags=flags, device=0)
    fs.set_mesh(xyz, tri, quad)
    fs.set_dirichlet(dmask)
    fs.set_loads(loads)
    fs.assemble()
    fs.set_preconditioner("amg", coarsest_nodes=coarsest_nodes)
    return fs


def level_operator(fs, level):
    """(rowptr, colidx, vals [nnzb, 6, 6]) of a level of the context's hierarchy: K from export_bsr, the coarse operators from amg_export"""
    if level == 0:
        r, c, v, _ = fs.export_bsr()
        return np.asarray(r, dtype=np.int64), c, v.reshape(-1, 6, 6)
    ex = fs.amg_export(level)
    return ex["A_rowptr"], ex["A_cols"], ex["A_vals"].reshape(-1, 6, 6)


# ---- the two readers -------------------------------------------------------------------------------------------------------------
def apply_truth(B, r):
    """(B r in long double, the bound 6 eps sum_j |B_ij| |r_j| per entry: six products and five additions of a dot product of
    six terms, (1 + eps/2)^6 - 1 < 6 eps / 2 with room for a fused or an unfused evaluation) for blocks B [n, 6, 6], r [n, 6]"""
    B, r = np.asarray(B).astype(LD), np.asarray(r).astype(LD)
    z = np.einsum("nij,nj->ni", B, r)
    budget = 6.0 * EPS * np.einsum("nij,nj->ni", np.abs(B), np.abs(r))
    return z, budget


# ---- the spectral bound -----------------------------------------------------------------------------------------------------------
def hash_vector(n_real, n_total=None):
    """k_fill_hash (csrc/amg_kernels.hip): entry i of the start vector of the power iteration, zero from n_real on"""
    n_total = n_real if n_total is None else n_total
    with np.errstate(over="ignore"):
        h = np.arange(n_total, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x2545F4914F6CDD1D)
        h ^= h >> np.uint64(29)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(32)
    u = (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    x = 2.0 * u - 1.0
    x[n_real:] = 0.0
    return x


def block_product(rowptr, colidx, vals, x):
    """A x for block CSR A and x [n, 6], in the precision of vals and x"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    y = np.zeros_like(x)
    np.add.at(y, rows, np.einsum("qij,qj->qi", vals, x[np.asarray(colidx)]))
    return y


def restated_lambda(rowptr, colidx, vals, Dinv, iterations=30, dtype=np.float64):
    """The power iteration of the setup (power_iteration_start / _finish), restated: x <- D^-1 A x from the hash vector without
    normalisation, `iterations` times; the ratio of the last two norms.  (Not yet multiplied by the safety factor.)"""
    n = len(rowptr) - 1
    vals = np.asarray(vals).reshape(-1, 6, 6).astype(dtype)
    Dinv = np.asarray(Dinv).astype(dtype)
    x = hash_vector(6 * n).reshape(n, 6).astype(dtype)
    norms = []
    for _ in range(max(iterations, 2)):
        x = np.einsum("nij,nj->ni", Dinv, block_product(rowptr, colidx, vals, x))
        norms.append(np.sqrt((x * x).sum()))
    return norms[-1] / norms[-2]


def dense_of(rowptr, colidx, vals):
    n = len(rowptr) - 1
    A = np.zeros((n, 6, n, 6))
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    A[rows, :, np.asarray(colidx), :] = np.asarray(vals).reshape(-1, 6, 6)
    return A.reshape(6 * n, 6 * n)


def true_lambda(rowptr, colidx, vals, labels=None):
    """lambda_max(D^-1 A), D the diagonal blocks of A, with no iteration involved: the largest eigenvalue of the pencil (A, D) by
    dense LAPACK.  D is block diagonal, so the pencil is reduced to standard form block by block -- C = L^-1 A L^-T with D_a = L_a
    L_a^T, Cholesky being as indifferent to the scaling of a shell block as the metric above -- and scipy.linalg.eigh takes the
    top of the spectrum of C (subset_by_index; its generalized driver with a subset, bisection and inverse iteration, gives up on
    the clustered eigenvalues these pencils have).
    labels (per node: its cluster of rigidly coupled nodes or -1, femshell_amg_export's patch_labels): the level smooths with one
    block per cluster (csrc/amg_patch.hpp), and D is the diagonal of A over THOSE blocks."""
    import scipy.linalg as sla

    n = len(rowptr) - 1
    A = dense_of(rowptr, colidx, vals)
    A = 0.5 * (A + A.T)
    if labels is not None and (np.asarray(labels) >= 0).any():
        labels = np.asarray(labels)
        group = np.where(labels >= 0, labels, labels.max() + 1 + np.arange(n))  # (a node outside every cluster: a block of its own)
        same = np.repeat(group, 6)
        D = np.where(same[:, None] == same[None, :], A, 0.0)
        L = np.linalg.cholesky(D)
        C = sla.solve_triangular(L, sla.solve_triangular(L, A, lower=True).T, lower=True)
    else:
        Linv = np.zeros((n, 6, 6))
        for a, blk in enumerate(diagonal_blocks(rowptr, colidx, vals)):
            Linv[a] = sla.solve_triangular(np.linalg.cholesky(0.5 * (blk + blk.T)), np.eye(6), lower=True)
        C = np.einsum("aij,ajbk->aibk", Linv, A.reshape(n, 6, n, 6))
        C = np.einsum("aibk,blk->aibl", C, Linv).reshape(6 * n, 6 * n)
    w = sla.eigh(0.5 * (C + C.T), eigvals_only=True, subset_by_index=[6 * n - 1, 6 * n - 1])
    return float(w[0])


def true_lambda_sparse(rowptr, colidx, vals, tol=1e-13):
    """The same number for an operator too large for a dense eigh (the 14,022 dofs of level 0 of the row-partitioned panel would
    take minutes): the top of the spectrum of the same C = L^-1 A L^-T, kept sparse, by scipy's implicitly restarted Lanczos
    run to convergence at `tol` -- an iteration, but not the one under test, and it stops on its own residual."""
    import scipy.sparse as sp
    import scipy.linalg as sla
    import scipy.sparse.linalg as spla

    n = len(rowptr) - 1
    vals = np.asarray(vals).reshape(-1, 6, 6)
    Linv = np.zeros((n, 6, 6))
    for a, blk in enumerate(diagonal_blocks(rowptr, colidx, vals)):
        Linv[a] = sla.solve_triangular(np.linalg.cholesky(0.5 * (blk + blk.T)), np.eye(6), lower=True)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    Cv = np.einsum("qij,qjk,qlk->qil", Linv[rows], vals, Linv[np.asarray(colidx)])
    C = sp.bsr_matrix((Cv, np.asarray(colidx), np.asarray(rowptr)), shape=(6 * n, 6 * n)).tocsr()
    C = 0.5 * (C + C.T)
    w = spla.eigsh(C, k=1, which="LA", tol=tol, ncv=40, return_eigenvectors=False)
    return float(w[0])
