"""Reference for ONE application of the multigrid preconditioner (femshell_pc_apply): an oracle/amg_oracle.py Level list built from
the hierarchy the library exports -- its level operators, prolongators, spectral bounds and coarsest inverse --, so that
amg_oracle.cycle() on it differs from the device's cycle by the solve-phase kernels alone (smoothers, transfers, the K cycle's
Krylov steps, the coarsest solve), not by the setup, which tests/test_gpu_amg.py holds to the restatement on its own.  CPU code.

float_mode mirrors the single-precision copies of csrc/amg_hierarchy.cpp (FEMSHELL_AMG_SMOOTH_F32, amg_finish_hierarchy) rule for
rule: on a level that keeps them the smoothing products and the residual increments read A rounded to float32 (L.As), the
smoother's block inverse is rounded to float32, P and R are rounded where the next level has at least 4096 nodes (every level
with mode 3, none with mode 2); the K cycle's products, the Galerkin operators and every vector stay FP64, and a level with
clusters of rigidly coupled nodes keeps everything FP64.  What FEMSHELL_AMG_VEC_F32 rounds besides (vectors of the
symmetric-storage products) is not modelled: the tests compare such runs against this values-only model with a wider tolerance."""
import numpy as np
import scipy.sparse as sp

from oracle import amg_oracle

# Tolerances of the comparisons of the device's cycle with this reference (measured values: tests/test_gpu_cycle.py)
TOL_FP64 = 5e-12  # FP64 levels
TOL_F32 = 1e-11   # single-precision copies of the values, FEMSHELL_AMG_VEC_F32=0, against the float model
TOL_VEC = 5e-6    # FEMSHELL_AMG_VEC_F32=1/2 against the values-only float model

DEFAULTS = {"smoother_degree": 3, "coarse_degree": 4, "eig_ratio": 30.0}  # csrc/amg_hierarchy.cpp amg_default_options
F32_MIN_NODES = 4096  # FEMSHELL_AMG_SMOOTH_F32=1: levels of at least this many nodes keep the copies


def bsr(rowptr, cols, vals, n_cols):
    n = len(rowptr) - 1
    return sp.bsr_matrix((np.asarray(vals).reshape(-1, 6, 6), cols, rowptr), shape=(6 * n, 6 * n_cols))


def to_f32(M):
    """M with its values rounded to single precision (a scipy matrix or an array)."""
    if sp.issparse(M):
        M = M.copy()
        M.data = M.data.astype(np.float32).astype(np.float64)
        return M
    return np.asarray(M).astype(np.float32).astype(np.float64)


def chebyshev(L, lam, degree, eig_ratio):
    """The smoother's coefficients of a level with spectral bound lam (csrc/amg_hierarchy.cpp amg_finish_hierarchy)."""
    lmax, lmin = lam, lam / eig_ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    L.lam = lam
    L.inv_theta = 1.0 / theta
    L.cheb = []
    rho = 1.0 / sigma
    for _ in range(1, max(1, degree)):
        rho_new = 1.0 / (2.0 * sigma - rho)
        L.cheb.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new


def build_levels(As, Ps, lams, coarse_inverse, opts=None, patch_labels=None, float_mode=0, f32_min_nodes=F32_MIN_NODES):
    """As[l]: level operators (scipy, FP64), Ps[l]: prolongators from level l + 1 (len(As) - 1 of them), lams[l]: spectral bounds,
    coarse_inverse: the dense inverse the cycle applies on the last level.  patch_labels: level 0's clusters (femshell_amg_export
    FEMSHELL_AMG_PATCH_LABELS).  Returns the Level list amg_oracle.cycle() takes."""
    o = dict(DEFAULTS, **(opts or {}))
    levels = []
    for l, A in enumerate(As):
        L = amg_oracle.Level()
        L.A = A.tobsr((6, 6))
        L.n = L.A.shape[0] // 6
        L.patch = None
        levels.append(L)
        if l + 1 == len(As):
            L.dense_inv = np.asarray(coarse_inverse, dtype=np.float64)
            break
        Dinv = amg_oracle.block_diag_inverse(L.A)
        Dinv = 0.5 * (Dinv + Dinv.transpose(0, 2, 1))  # (the device keeps the symmetric inverse: 21 values per node)
        L.Dinv = Dinv
        L.Dm = amg_oracle.bd_matrix(Dinv)
        if l == 0 and patch_labels is not None and np.any(np.asarray(patch_labels) >= 0):
            label = np.asarray(patch_labels, dtype=np.int64)
            nc = int(label.max()) + 1
            ptr = np.concatenate([[0], np.cumsum(np.bincount(label[label >= 0], minlength=nc))]).astype(np.int64)
            nodes = np.flatnonzero(label >= 0)[np.argsort(label[label >= 0], kind="stable")]
            L.Dm = amg_oracle.patch_block_inverse(L.A, Dinv, label, ptr, nodes)
            L.patch = (label, L.Dm)
        L.P = Ps[l].tobsr((6, 6))
        L.R = L.P.T.tobsr((6, 6))
        chebyshev(L, lams[l], o["smoother_degree"] if l == 0 else o["coarse_degree"], o["eig_ratio"])
    apply_float_copies(levels, float_mode, f32_min_nodes)
    return levels


def apply_float_copies(levels, mode, f32_min_nodes=F32_MIN_NODES):
    """The single-precision copies of FEMSHELL_AMG_SMOOTH_F32 = mode (0 off, 1 levels of at least f32_min_nodes nodes, 2 level 0
    only, 3 every level), rule for rule as csrc/amg_hierarchy.cpp sets them up.  Returns the indices of the levels that got them."""
    got = []
    for l, L in enumerate(levels[:-1]):
        if mode == 0 or (mode == 2 and l > 0) or (mode == 1 and L.n < f32_min_nodes) or L.patch is not None:
            continue
        L.As = to_f32(L.A)
        L.Dm = amg_oracle.bd_matrix(to_f32(L.Dinv))
        big_coarse = mode == 3 or levels[l + 1].n >= f32_min_nodes
        if mode != 2 and big_coarse:
            L.P = to_f32(L.P)
            L.R = L.P.T.tobsr((6, 6))  # (R = P^T value by value: the rounded pair is still a transposed pair)
        got.append(l)
    return got


def internal_order(fs, A0_internal):
    """perm[internal row] = the caller's node of that row, found by matching the diagonal blocks of K in the caller's numbering
    (femshell_export_bsr) with those of level 0 of the hierarchy (internal numbering); None when the two numberings agree.  Needs
    a mesh whose diagonal blocks are all different (an unstructured one).  (The library exports no permutation: the renumbering is
    internal to a context, and an entry point that hands it out for tests alone would be API to keep for nothing else.  The
    blocks identify the rows exactly because the two exports hold the very same values; the assertion below stops a mesh where
    they do not.)"""
    rg, cg, vg, _ = fs.export_bsr()
    Kc = bsr(rg, cg, vg, len(rg) - 1)
    if (Kc != A0_internal).nnz == 0:
        return None
    dc = amg_oracle.block_diag(Kc).reshape(len(rg) - 1, -1)
    di = amg_oracle.block_diag(A0_internal).reshape(len(rg) - 1, -1)
    key_c = {}
    for i in range(len(dc)):
        key_c.setdefault(dc[i].tobytes(), []).append(i)
    # (nodes with all six dofs fixed: multiples of the unit block, decoupled from the rest -- any order among them serves)
    fixed = lambda k: np.array_equal(np.frombuffer(k).reshape(6, 6), np.frombuffer(k)[0] * np.eye(6))  # noqa: E731
    assert all(len(v) == 1 for k, v in key_c.items() if not fixed(k)), "diagonal blocks are not unique: no numbering can be read off them"
    perm = np.array([key_c[di[j].tobytes()].pop(0) for j in range(len(di))], dtype=np.int64)
    assert len(np.unique(perm)) == len(perm)
    return perm


def levels_from_context(fs, opts=None, float_mode=0, f32_min_nodes=F32_MIN_NODES):
    """The Level list of the hierarchy of a single-rank context (after a solve or a pc_apply), in its internal numbering, and the
    permutation from internal rows to the caller's nodes (None: the same numbering)."""
    lv = fs.amg_levels()
    assert len(lv) >= 2
    As, Ps = [], []
    for l in range(len(lv)):
        ex = fs.amg_export(l)
        assert ex["A_vals"] is not None, "level %d has no host copy" % l
        As.append(bsr(ex["A_rowptr"], ex["A_cols"], ex["A_vals"], lv[l]["n_nodes"]))
        if l + 1 < len(lv):
            Ps.append(bsr(ex["P_rowptr"], ex["P_cols"], ex["P_vals"], lv[l]["n_coarse"]))
        else:
            inv = ex["coarse_inverse"]
        if l == 0:
            labels = ex["patch_labels"]
    levels = build_levels(As, Ps, [x["lambda_max"] for x in lv], inv, opts, labels, float_mode, f32_min_nodes)
    return levels, internal_order(fs, As[0])


def apply(levels, r, kcycle, perm=None):
    """z = M^-1 r of the reference; r, z in the caller's numbering when perm (internal row -> caller's node) is given."""
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    if perm is None:
        return amg_oracle.cycle(levels, 0, r, kcycle)
    ri = r.reshape(-1, 6)[perm].ravel()
    zi = amg_oracle.cycle(levels, 0, ri, kcycle)
    z = np.empty_like(zi)
    z.reshape(-1, 6)[perm] = zi.reshape(-1, 6)
    return z


def free_dofs(fs):
    """Mask of the dofs of K (the caller's numbering) that are not Dirichlet rows -- a Dirichlet row holds its unit diagonal
    only, and its entry of M^-1 r is that of r, seven decades above the others: inputs are zero there, so that the comparisons
    measure the rest."""
    rg, cg, vg, _ = fs.export_bsr()
    K = bsr(rg, cg, vg, len(rg) - 1).tocsr()
    K.eliminate_zeros()
    return ~((K.getnnz(axis=1) == 1) & (K.diagonal() == 1.0))


def errors(z, z_ref):
    """(||z - z_ref|| / ||z_ref||, worst node: max over nodes of ||z_i - z_ref_i|| / max over nodes of ||z_ref_i||)."""
    d = (np.asarray(z) - np.asarray(z_ref)).reshape(-1, 6)
    zr = np.asarray(z_ref).reshape(-1, 6)
    rel = np.linalg.norm(d) / np.linalg.norm(zr)
    node = np.linalg.norm(d, axis=1).max() / np.linalg.norm(zr, axis=1).max()
    return float(rel), float(node)
