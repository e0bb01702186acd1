"""Load cases (femshell_solve_cases; csrc/cases.cpp, cases.hip): a numpy restatement of the lockstep recurrence in long double.

Several right-hand sides on one K run the classic block-Jacobi CG side by side in passes of `pass_cols` columns; every column has
its own scalars (alpha, beta, r.z, r.r, b.b, the threshold, iterations, done), and a column whose done flag is set is frozen: no
kernel reads or writes it again.  `scalar_step` restates the branch thread 0 of k_cases_scalar takes, as krylov_truth.scalar_phase
restates cg_scalar_phase; `lockstep` restates cases_lockstep_cg with the vector kernels as whole-vector numpy operations.  The sums
are plain dots in `dtype`: how the device groups its partial sums is not restated (a bound on that is what the GPU tests assert).

DEFECTS are planted into the restatement by name; tests/test_load_cases_cpu.py shows that each is caught by the checks the GPU
tests run on the device: the dense solve and the independence of a column from its company."""
import numpy as np

LD = np.longdouble
INIT, ALPHA, BETA = 1, 2, 3

# update_after_done: the vector kernels do not look at the done flag -- a finished column keeps taking x += alpha p, r -= alpha q
#     with the alpha it finished with while its neighbours run
# alpha_of_column_0: the update of column 1 of a pass reads the alpha of column 0
# tail_pass_fifth_column: the tail pass takes its columns at passes * nb instead of passes * pass_cols -- with five cases it solves
#     the second column again and never reads the fifth
DEFECTS = ("update_after_done", "alpha_of_column_0", "tail_pass_fifth_column")


class Column:
    """CaseScalars of csrc/cases.hpp"""

    def __init__(self, dtype=LD):
        z = dtype(0.0)
        self.rz = self.alpha = self.beta = self.rr = self.bb = self.tol2 = self.pq = z
        self.done = 0
        self.iters = 0

    def info(self):
        rel = float(np.sqrt(self.rr / self.bb)) if self.bb > 0 else 0.0
        return {"iterations": self.iters, "converged": self.done, "rel_residual": rel}


def scalar_step(phase, s, red, rtol):
    """thread 0 of k_cases_scalar for one column: red = the column's sums (INIT: r.z, b.b; ALPHA: p.q; BETA: r.z, r.r).  Returns
    False where the kernel returns before the sums (a frozen column)."""
    if phase != INIT and s.done != 0:
        return False
    dtype = type(s.rz)
    rtol = dtype(rtol)
    with np.errstate(all="ignore"):
        if phase == INIT:
            s.rz, s.bb, s.rr = red[0], red[1], red[1]
            s.tol2 = rtol * rtol * red[1] if rtol > 0 else dtype(0.0)
            s.alpha = s.beta = s.pq = dtype(0.0)
            s.iters = 0
            s.done = 1 if red[1] == 0 else 0
        elif phase == ALPHA:
            s.pq = red[0]
            if not red[0] > 0:
                s.done = -1
            else:
                s.alpha = s.rz / red[0]
        elif phase == BETA:
            s.rr = red[1]
            s.iters += 1
            if red[1] <= s.tol2:
                s.done = 1
            else:
                s.beta = red[0] / s.rz
                s.rz = red[0]
        else:
            raise ValueError(phase)
    return True


def lockstep(A, Minv, B, rtol, max_it, pass_cols=4, dtype=LD, defect=None):
    """cases_lockstep_cg: A (n, n) and B (n_cases, n), the masked loads; Minv: r -> D^-1 r in `dtype`.  Returns (X (n_cases, n) in
    `dtype`, the Columns, passes).  The host's polling is not restated: it ends a pass when every further launch would be a
    no-op."""
    assert defect is None or defect in DEFECTS, defect
    A = np.asarray(A, dtype=dtype)
    B = np.asarray(B, dtype=dtype)
    n_cases, n = B.shape
    X = np.zeros((n_cases, n), dtype=dtype)
    R = B.copy()
    cols = [Column(dtype) for _ in range(n_cases)]
    passes = 0
    j0 = 0
    while j0 < n_cases:
        nb = min(pass_cols, n_cases - j0)
        first = j0
        if defect == "tail_pass_fifth_column" and nb < pass_cols:
            first = passes * nb
        idx = list(range(first, first + nb))
        Z = np.zeros((nb, n), dtype=dtype)
        P = np.zeros((nb, n), dtype=dtype)
        for k, j in enumerate(idx):  # k_cases_init
            X[j] = 0
            Z[k] = Minv(R[j])
            P[k] = Z[k]
            scalar_step(INIT, cols[j], (R[j] @ Z[k], R[j] @ R[j]), rtol)
        for _ in range(max_it):
            if all(cols[j].done != 0 for j in idx):
                break
            # the block product: every column, frozen or not (column by column: a matrix-matrix product of the BLAS behind numpy
            # rounds a column differently with its company, which k_spmm_sym does not)
            Q = np.stack([A @ P[k] for k in range(nb)])
            for k, j in enumerate(idx):  # k_cases_dot + the scalar step
                if cols[j].done == 0:
                    scalar_step(ALPHA, cols[j], (P[k] @ Q[k],), rtol)
            for k, j in enumerate(idx):  # k_cases_update + the scalar step
                s = cols[j]
                if s.done != 0 and defect != "update_after_done":
                    continue
                alpha = s.alpha
                if defect == "alpha_of_column_0" and k == 1:
                    alpha = cols[idx[0]].alpha
                X[j] = X[j] + alpha * P[k]
                R[j] = R[j] - alpha * Q[k]
                Z[k] = Minv(R[j])
                scalar_step(BETA, s, (R[j] @ Z[k], R[j] @ R[j]), rtol)
            for k, j in enumerate(idx):  # k_cases_direction
                if cols[j].done == 0:
                    P[k] = Z[k] + cols[j].beta * P[k]
        passes += 1
        j0 += nb
    return X, cols, passes


# ------------------------------------------------------------------ operators

def dense_from_bsr(rowptr, colidx, vals, dtype=np.float64):
    """the (6 n, 6 n) matrix of a block CSR with 6 x 6 blocks"""
    n = len(rowptr) - 1
    K = np.zeros((6 * n, 6 * n), dtype=dtype)
    vals = np.asarray(vals).reshape(-1, 6, 6)
    for a in range(n):
        for k in range(rowptr[a], rowptr[a + 1]):
            c = colidx[k]
            K[6 * a:6 * a + 6, 6 * c:6 * c + 6] = vals[k]
    return K


def block_jacobi(K, dtype=LD):
    """r -> D^-1 r with the inverses of the 6 x 6 diagonal blocks of K, formed in float64 and applied in `dtype`"""
    n = K.shape[0] // 6
    inv = np.stack([np.linalg.inv(np.asarray(K[6 * a:6 * a + 6, 6 * a:6 * a + 6], dtype=np.float64)) for a in range(n)]).astype(dtype)
    inv = 0.5 * (inv + inv.transpose(0, 2, 1))

    def apply(r):
        return np.einsum("aij,aj->ai", inv, np.asarray(r, dtype=dtype).reshape(n, 6)).reshape(-1)

    return apply


def dense_solve(K, B):
    """K^-1 B^T by LU in float64 with refinement sweeps whose residual is taken in long double: (n_cases, n) in long double"""
    K64 = np.asarray(K, dtype=np.float64)
    KL = np.asarray(K, dtype=LD)
    BL = np.asarray(B, dtype=LD)
    X = np.linalg.solve(K64, np.asarray(B, dtype=np.float64).T).T.astype(LD)
    for _ in range(4):
        Rr = BL - X @ KL.T
        X = X + np.linalg.solve(K64, Rr.astype(np.float64).T).T.astype(LD)
    return X


def mask_of(n):
    """partly fixed nodes all over the mesh, one node clamped: K is positive definite and no dof class is left alone"""
    mask = np.zeros(n, np.uint8)
    mask[::3] = 0x15
    mask[0] = 0x3F
    return mask


def mask_for(name, n):
    """The Dirichlet set the GPU tests put on the device mesh `name` (tests/helpers/resultants.py device_meshes).  mask_of, but for
    the Delaunay patch: its triangles go down to a quality of 0.007 (edges of 0.003 beside a thickness of 0.37).  Under mask_of
    the block-Jacobi CG of the CPU oracle needs 8087 iterations to 1e-12 for 2997 unknowns, 3673 to 1e-2 -- past the count at
    which CG ends in exact arithmetic.  With every second node clamped it needs about 380 for 1500 unknowns, but its own count
    moves between 371 and 390 when the load is multiplied by 1 + 2^-40, 3, 1/3 or 0.7 (perturbations of the size of a rounding):
    the last digits are reached through a plateau, and no bar of +-3 on a difference of counts means anything there
    (femshell_solve and the oracle differ by 13).  With three of four nodes clamped the oracle needs 197 .. 201 iterations for
    1125 unknowns and moves by at most 2 under the same perturbations, at 1e-8 and 1e-10 too: the set used here.  The tests
    assert what they can of the condition: no more iterations than unknowns."""
    if not name.startswith("delaunay"):
        return mask_of(n)
    mask = np.full(n, 0x3F, np.uint8)
    mask[1::4] = 0
    mask[3::8] = 0x15
    return mask


def free_dofs(mask):
    return ((np.asarray(mask, np.uint8)[:, None] >> np.arange(6)) & 1).reshape(-1) == 0


def case_loads(n_nodes, mask, n_cases, seed=11):
    """(n_cases, n_nodes, 6): seeded random loads of different sizes, with the second case a load on a single free node and, from
    three cases on, the third all zero"""
    rng = np.random.default_rng(seed)
    L = rng.uniform(-1.0, 1.0, (n_cases, n_nodes, 6)) * (10.0 ** rng.integers(-2, 3, n_cases))[:, None, None]
    if n_cases > 1:
        node = int(np.flatnonzero(np.asarray(mask) == 0)[len(np.flatnonzero(np.asarray(mask) == 0)) // 2])
        L[1] = 0.0
        L[1, node, :3] = (0.3, -1.0, 0.7)
    if n_cases > 2:
        L[2] = 0.0
    return L
